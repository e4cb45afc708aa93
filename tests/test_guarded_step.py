"""CPU: the guarded optimizer step (FlatAdamW(skip_nonfinite=True)) as far as it goes without a GPU -- the C ABI (symbols, the
dvla_step_state mirror against gcc, argument checks that return before any launch), the host-derived candidate scalars against
a Python restatement of the expressions in dvla_adamw_bf16 / dvla_adamw_f32_master, and the ledger that decides which step
counts a step may need (optim._StepLedger) against a scripted device."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dvla_step_candidates", "dvla_step_verdict", "dvla_adamw_bf16_guarded", "dvla_adamw_f32_master_guarded"]
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def test_symbols_are_bound_and_the_abi_version_stays():
    from dreamvla_amd import _lib
    assert all(s in _lib.SYMBOLS for s in NEW)
    assert _lib.ABI_VERSION == 9
    lib = _lib.load()
    assert lib.dvla_abi_version() == 9 and all(hasattr(lib, s) for s in NEW)
    txt = open(os.path.join(ROOT, "include", "dvla.h")).read()
    assert re.search(r"#define DVLA_ABI_VERSION 9\b", txt)


def test_flat_adamw_accepts_skip_nonfinite_defaulting_to_off():
    from dreamvla_amd.optim import FlatAdamW
    par = inspect.signature(FlatAdamW.__init__).parameters
    assert "skip_nonfinite" in par and par["skip_nonfinite"].default is False


def test_step_state_mirror_matches_the_c_compiler(tmp_path):
    from dreamvla_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    structs = {"dvla_step_state": _lib.StepState, "dvla_step_scalars": _lib.StepScalars}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dvla.h"', 'int main(void) {',
             '  printf("max buckets %d\\n", DVLA_STEP_MAX_BUCKETS);', '  printf("max candidates %d\\n", DVLA_STEP_MAX_CANDIDATES);',
             '  printf("dvla_step_state alignof %zu\\n", (size_t)__alignof__(dvla_step_state));']
    for cname, py in structs.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).strip().splitlines():
        cname, field, val = line.split()
        if cname == "max":
            assert int(val) == {"buckets": _lib.STEP_MAX_BUCKETS, "candidates": _lib.STEP_MAX_CANDIDATES}[field]
        elif field == "alignof":
            assert int(val) == 16
        else:
            py = structs[cname]
            want = ctypes.sizeof(py) if field == "sizeof" else getattr(py, field).offset
            assert int(val) == want, f"{cname}.{field}: C {val} vs ctypes {want}"
        seen += 1
    assert seen == 3 + 2 + len(_lib.StepState._fields_) + len(_lib.StepScalars._fields_)
    assert ctypes.sizeof(_lib.StepState) % 16 == 0
    # the per-step readback is the head of the struct: the counters, the verdict and the norm
    head = [f for f, _ in _lib.StepState._fields_ if getattr(_lib.StepState, f).offset < _lib.STEP_READBACK_BYTES]
    assert head == ["applied", "skipped", "faults", "ok", "sumsq"] and _lib.StepState.cand.offset == _lib.STEP_READBACK_BYTES


def _aligned_host_buffer(nbytes):
    raw = (ctypes.c_uint8 * (nbytes + 16))()
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_new_entry_points_check_their_arguments_before_any_launch():
    """host memory stands in for device memory: every call below must return before it launches anything"""
    from dreamvla_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_host_buffer(4096)
    cand = (_lib.StepScalars * 9)()
    # dvla_step_candidates
    assert lib.dvla_step_candidates(1e-3, 0.9, 0.999, 1, 9, None) == ERR_ARG
    assert lib.dvla_step_candidates(1e-3, 0.9, 0.999, 0, 9, cand) == ERR_ARG
    assert lib.dvla_step_candidates(1e-3, 0.9, 0.999, 1, 0, cand) == ERR_ARG
    assert lib.dvla_step_candidates(1e-3, 0.9, 0.999, 1, 10, cand) == ERR_ARG
    assert lib.dvla_step_candidates(1e-3, 0.9, 0.999, 1, 9, cand) == 0
    # dvla_step_verdict(bucket_sumsq, n, grad_sumsq, state, confirmed_applied, n_cand, cand, stream)
    assert lib.dvla_step_verdict(None, 2, p, p, 0, 1, cand, None) == ERR_ARG
    assert lib.dvla_step_verdict(p, 2, None, p, 0, 1, cand, None) == ERR_ARG
    assert lib.dvla_step_verdict(p, 2, p, None, 0, 1, cand, None) == ERR_ARG
    assert lib.dvla_step_verdict(p, 2, p, p, 0, 1, None, None) == ERR_ARG
    assert lib.dvla_step_verdict(p, -1, p, p, 0, 1, cand, None) == ERR_ARG
    assert lib.dvla_step_verdict(p, 2, p, p, -1, 1, cand, None) == ERR_ARG
    assert lib.dvla_step_verdict(p, 2, p, p, 0, 0, cand, None) == ERR_ARG
    assert lib.dvla_step_verdict(p, 2, p, p, 0, 10, cand, None) == ERR_ARG
    assert lib.dvla_step_verdict(p, _lib.STEP_MAX_BUCKETS + 1, p, p, 0, 1, cand, None) == ERR_UNSUPPORTED
    assert lib.dvla_step_verdict(p, 2, p, p + 8, 0, 1, cand, None) == ERR_UNSUPPORTED
    assert lib.dvla_step_verdict(p, 0, p, p, 0, 1, cand, None) == 0
    # dvla_adamw_bf16_guarded(param, grad, m, v, n, lr, beta1, beta2, eps, wd, max_norm, state, stream)
    hp = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.1)
    for k in range(4):
        ptrs = [p, p, p, p]
        ptrs[k] = None
        assert lib.dvla_adamw_bf16_guarded(*ptrs, 8, *hp, p, None) == ERR_ARG
        ptrs[k] = p + 2
        assert lib.dvla_adamw_bf16_guarded(*ptrs, 8, *hp, p, None) == ERR_UNSUPPORTED
    assert lib.dvla_adamw_bf16_guarded(p, p, p, p, 8, *hp, None, None) == ERR_ARG
    assert lib.dvla_adamw_bf16_guarded(p, p, p, p, -1, *hp, p, None) == ERR_ARG
    assert lib.dvla_adamw_bf16_guarded(p, p, p, p, 8, *hp, p + 4, None) == ERR_UNSUPPORTED
    assert lib.dvla_adamw_bf16_guarded(p, p, p, p, 0, *hp, p, None) == 0
    # dvla_adamw_f32_master_guarded(param, grad, m, v, shadow, n, lr, beta1, beta2, eps, wd, max_norm, state, stream)
    for k in range(4):
        ptrs = [p, p, p, p]
        ptrs[k] = None
        assert lib.dvla_adamw_f32_master_guarded(*ptrs, p, 8, *hp, p, None) == ERR_ARG
        ptrs[k] = p + 4
        assert lib.dvla_adamw_f32_master_guarded(*ptrs, p, 8, *hp, p, None) == ERR_UNSUPPORTED
    assert lib.dvla_adamw_f32_master_guarded(p, p, p, p, p, 8, *hp, None, None) == ERR_ARG
    assert lib.dvla_adamw_f32_master_guarded(p, p, p, p, p, -1, *hp, p, None) == ERR_ARG
    assert lib.dvla_adamw_f32_master_guarded(p, p, p, p, p + 2, 8, *hp, p, None) == ERR_UNSUPPORTED
    assert lib.dvla_adamw_f32_master_guarded(p, p, p, p, p, 8, *hp, p + 8, None) == ERR_UNSUPPORTED
    assert lib.dvla_adamw_f32_master_guarded(p, p, p, p, None, 0, *hp, p, None) == 0
    del keep


def _f32(x):
    return ctypes.c_float(x).value


def _restated_scalars(lr, beta1, beta2, step):
    """the lines of dvla_adamw_bf16 (betas arrive as floats) and of dvla_adamw_f32_master (doubles), in Python doubles"""
    b1f, b2f = _f32(beta1), _f32(beta2)
    bc1, bc2 = 1.0 - b1f ** step, 1.0 - b2f ** step
    inv_bc1, inv_bc2_sqrt = _f32(1.0 / bc1), _f32(1.0 / math.sqrt(bc2))
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return inv_bc1, inv_bc2_sqrt, _f32(bc2 ** 0.5), _f32((lr / bc1) * -1.0)


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.9, 0.95)])
@pytest.mark.parametrize("base", [1, 5, 1000])
def test_candidates_equal_the_restated_expressions_float_for_float(betas, base):
    from dreamvla_amd import _lib
    lib = _lib.load()
    lr = 1e-3
    cand = (_lib.StepScalars * 9)()
    assert lib.dvla_step_candidates(lr, betas[0], betas[1], base, 9, cand) == 0
    for j in range(9):
        got = (cand[j].inv_bc1, cand[j].inv_bc2_sqrt, cand[j].bc2_sqrt, cand[j].step_size)
        assert got == _restated_scalars(lr, betas[0], betas[1], base + j), (base + j, got)
    # a shorter table fills only its rows
    short = (_lib.StepScalars * 9)()
    assert lib.dvla_step_candidates(lr, betas[0], betas[1], base, 3, short) == 0
    assert [short[j].step_size for j in range(9)] == [cand[j].step_size for j in range(3)] + [0.0] * 6


# ----------------------------------------------------------------------------------------------------------------------------
# the ledger against a scripted device
# ----------------------------------------------------------------------------------------------------------------------------
class _Ticket:
    def __init__(self, dev, index, readback):
        self.dev, self.index, self.readback, self.is_done = dev, index, readback, False

    def done(self):
        return self.is_done

    def wait(self):
        self.dev.waits.append(self.index)
        self.is_done = True

    def read(self):
        assert self.is_done, "the ledger read a readback that had not arrived"
        return self.readback


class _Device:
    """what dvla_step_verdict does to the counters, step by step, and when each readback arrives (the test decides)"""

    def __init__(self, ledger, applied=0, skipped=0):
        self.ledger, self.applied, self.skipped, self.faults = ledger, applied, skipped, 0
        self.tickets, self.waits, self.used = [], [], []

    def step(self, ok, faults=0):
        confirmed, n_cand = self.ledger.begin()
        cands = self.ledger.candidates()
        assert len(cands) == n_cand <= 9 and cands == [confirmed + 1 + j for j in range(n_cand)]
        assert self.applied + 1 in cands, (self.applied + 1, cands)          # the step count this step really needs
        self.used.append(self.applied + 1)
        self.applied += bool(ok)
        self.skipped += not ok
        self.faults += faults
        t = _Ticket(self, len(self.tickets), (self.applied, self.skipped, self.faults, int(bool(ok)), 1.0 if ok else math.inf))
        self.tickets.append(t)
        self.ledger.issued(t)
        return cands

    def arrive(self, *indices):
        for i in indices:
            self.tickets[i].is_done = True


def _ledger(**kw):
    from dreamvla_amd.optim import _StepLedger
    return _StepLedger(**kw)


def test_ledger_without_skips_in_lock_step():
    led = _ledger()
    dev = _Device(led)
    for k in range(1, 6):
        assert dev.step(True) == [k]
        dev.arrive(k - 1)
    assert dev.waits == [] and led.inflight == 1
    led.drain()
    assert (led.confirmed_applied, led.confirmed_skipped, led.inflight) == (5, 0, 0)


def test_ledger_skip_confirmed_late():
    skipped = []
    led = _ledger(on_skip=skipped.append)
    dev = _Device(led)
    assert dev.step(True) == [1]
    assert dev.step(False) == [1, 2]            # step 1 not confirmed yet: this one is count 1 or 2 (it is 2, and is skipped)
    assert dev.step(True) == [1, 2, 3]          # really count 2: the skip did not advance it
    assert dev.used == [1, 2, 2] and skipped == []
    dev.arrive(0, 1, 2)
    assert dev.step(True) == [3]
    assert skipped == [2] and (led.confirmed_applied, led.confirmed_skipped) == (2, 1)
    assert dev.waits == []


def test_ledger_ninth_step_waits_for_the_oldest_readback_only():
    led = _ledger()
    dev = _Device(led)
    for k in range(8):
        assert dev.step(k != 3) == list(range(1, k + 2))
    assert led.inflight == 8 and dev.waits == []
    cands = dev.step(True)
    assert dev.waits == [0]                      # the oldest, nothing else
    assert cands == list(range(2, 10)) and led.inflight == 8
    dev.step(True)
    assert dev.waits == [0, 1]
    led.drain()
    assert dev.waits == list(range(10)) and (led.confirmed_applied, led.confirmed_skipped) == (9, 1)


def test_ledger_retires_in_order_whatever_arrives_first():
    led = _ledger()
    dev = _Device(led)
    dev.step(True), dev.step(False), dev.step(True)
    dev.arrive(2)                                # the newest first: nothing can be retired
    assert dev.step(True) == [1, 2, 3, 4] and led.inflight == 4
    dev.arrive(0)                                # now the oldest, but not the one behind it
    assert dev.step(False) == [2, 3, 4, 5] and led.inflight == 4
    dev.arrive(1)                                # 1 and 2 retire together; 3 and 4 stay
    assert dev.step(True) == [3, 4, 5] and led.confirmed_applied == 2 and led.confirmed_skipped == 1
    assert dev.waits == [] and dev.used == [1, 2, 2, 3, 4, 4]


def test_ledger_raises_on_a_faults_readback():
    led = _ledger()
    dev = _Device(led)
    dev.step(True)
    dev.step(False, faults=1)
    dev.arrive(0, 1)
    with pytest.raises(RuntimeError, match="outside"):
        led.begin()
    led2 = _ledger()
    dev2 = _Device(led2)
    dev2.step(False, faults=1)
    with pytest.raises(RuntimeError):
        led2.drain()


def test_ledger_reset_restarts_from_loaded_counts():
    led = _ledger()
    dev = _Device(led)
    dev.step(True), dev.step(True)
    led.reset(applied=7, skipped=2)              # what load_state_dict does
    assert (led.inflight, led.confirmed_applied, led.confirmed_skipped) == (0, 7, 2)
    dev = _Device(led, applied=7, skipped=2)
    assert dev.step(True) == [8]
    assert dev.step(False) == [8, 9]
    led.drain()
    assert (led.confirmed_applied, led.confirmed_skipped) == (8, 3)
