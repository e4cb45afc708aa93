"""CPU: FlatAdamW(ema_decay=...) as far as it goes without a GPU -- the seven new symbols, the ABI version that stays, the one
place the EMA weight is derived (dvla_ema_weights) against a Python restatement in doubles, argument checks that return before
any launch, and the constructor's validation, which comes before anything touches the reducer."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dvla_ema_weights", "dvla_adamw_f32_master_ema", "dvla_adamw_bf16_ema", "dvla_adamw_f32_master_ema_guarded",
       "dvla_adamw_bf16_ema_guarded", "dvla_ema_swap_f32", "dvla_ema_swap_bf16"]
ERR_ARG, ERR_UNSUPPORTED = -1, -3
MAX_CAND = 9


def test_symbols_are_bound_and_the_abi_version_stays():
    from dreamvla_amd import _lib
    assert len(NEW) == 7 and all(s in _lib.SYMBOLS for s in NEW)
    assert _lib.ABI_VERSION == 9
    lib = _lib.load()
    assert lib.dvla_abi_version() == 9 and all(hasattr(lib, s) for s in NEW)
    txt = open(os.path.join(ROOT, "include", "dvla.h")).read()
    assert re.search(r"#define DVLA_ABI_VERSION 9\b", txt)
    assert all(re.search(r"\b%s\s*\(" % s, txt) for s in NEW)
    assert _lib.STEP_MAX_CANDIDATES == MAX_CAND


def test_flat_adamw_accepts_ema_arguments_defaulting_to_off():
    from dreamvla_amd.optim import FlatAdamW
    par = inspect.signature(FlatAdamW.__init__).parameters
    assert par["ema_decay"].default is None and par["ema_warmup"].default is False
    for name in ("ema_weights", "ema_reset", "ema_state_dict", "load_ema_state_dict", "ema_model_state_dict"):
        assert callable(getattr(FlatAdamW, name))


def _f32(x):
    return ctypes.c_float(x).value


def _d(decay, warmup, t):
    """the decay of applied step t (1-based), in Python doubles"""
    return min(decay, (1 + t) / (10 + t)) if warmup else decay


def _table(lib, decay, warmup, base, n):
    out = (ctypes.c_float * MAX_CAND)(*([-1.0] * MAX_CAND))
    assert lib.dvla_ema_weights(decay, int(warmup), base, n, out) == 0
    return list(out)


@pytest.mark.parametrize("warmup", [False, True], ids=["flat", "warmup"])
@pytest.mark.parametrize("decay", [0.5, 0.999, 0.9999])
def test_weights_equal_the_restated_expression_bit_for_bit(decay, warmup):
    from dreamvla_amd import _lib
    lib = _lib.load()
    for base in range(1, 41):
        got = _table(lib, decay, warmup, base, MAX_CAND)
        want = [_f32(1.0 - _d(decay, warmup, base + j)) for j in range(MAX_CAND)]
        assert got == want, (base, got, want)
    # a shorter table fills only its rows
    assert _table(lib, decay, warmup, 3, 2)[2:] == [-1.0] * (MAX_CAND - 2)
    assert _table(lib, decay, warmup, 3, 0) == [-1.0] * MAX_CAND


def test_the_warmup_crosses_one_half_at_step_eight_which_takes_the_large_weight_branch():
    """ATen's lerp takes fma(w, diff, e) for |w| < 0.5 and fma(-diff, 1 - w, p) otherwise.  (1 + t) / (10 + t) is exactly 0.5 at
    t = 8: w(8) = 0.5, which is NOT below 0.5 -- the second branch; t = 7 lies above (second branch), t = 9 below (first)."""
    from dreamvla_amd import _lib
    lib = _lib.load()
    for decay in (0.999, 0.9999):
        w = _table(lib, decay, True, 1, MAX_CAND)        # t = 1 .. 9
        w7, w8, w9 = w[6], w[7], w[8]
        assert w7 == _f32(1.0 - 8.0 / 17.0) and w7 > 0.5
        assert w8 == 0.5 and not abs(w8) < 0.5
        assert w9 == _f32(1.0 - 10.0 / 19.0) and w9 < 0.5
        assert all(x >= 0.5 for x in w[:8]) and all(b < a for a, b in zip(w, w[1:]))
        # far along the ramp the decay takes over: (1 + t) / (10 + t) >= 0.999 from t = 8990
        far = _table(lib, decay, True, 100000, 1)[0]
        assert far == _f32(1.0 - decay)
    assert _table(lib, 0.5, True, 8, 3)[:3] == [0.5, 0.5, 0.5]     # min(0.5, 9/18), min(0.5, 10/19), ...


def _aligned_host_buffer(nbytes):
    raw = (ctypes.c_uint8 * (nbytes + 16))()
    return raw, (ctypes.addressof(raw) + 15) & ~15


def test_ema_weights_rejects_bad_arguments():
    from dreamvla_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_float * (MAX_CAND + 1))()
    assert lib.dvla_ema_weights(0.999, 0, 1, MAX_CAND + 1, out) == ERR_ARG
    assert lib.dvla_ema_weights(0.999, 0, 0, 1, out) == ERR_ARG
    assert lib.dvla_ema_weights(0.999, 0, 1, 1, None) == ERR_ARG
    assert lib.dvla_ema_weights(0.999, 0, 1, -1, out) == ERR_ARG
    for bad in (0.0, 1.0, -0.1, float("nan")):
        assert lib.dvla_ema_weights(bad, 0, 1, 1, out) == ERR_ARG
    assert lib.dvla_ema_weights(0.999, 0, 1, MAX_CAND, out) == 0


def test_new_entry_points_check_their_arguments_before_any_launch():
    """host memory stands in for device memory: every call below must return before it launches anything"""
    from dreamvla_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_host_buffer(4096)
    w = (ctypes.c_float * MAX_CAND)()
    hp = (1e-3, 0.9, 0.999, 1e-8, 1e-2)
    # dvla_adamw_bf16_ema(param, grad, m, v, ema, n, lr, beta1, beta2, eps, wd, step, grad_sumsq, max_norm, ema_w, stream)
    # dvla_adamw_bf16_ema_guarded(param, grad, m, v, ema, n, lr, beta1, beta2, eps, wd, max_norm, state, ema_w, n_cand, stream)
    for k in range(5):
        ptrs = [p] * 5
        ptrs[k] = None
        assert lib.dvla_adamw_bf16_ema(*ptrs, 8, *hp, 1, None, 0.0, 0.001, None) == ERR_ARG
        assert lib.dvla_adamw_bf16_ema_guarded(*ptrs, 8, *hp, 0.1, p, w, 1, None) == ERR_ARG
        ptrs[k] = p + (4 if k == 4 else 2)
        assert lib.dvla_adamw_bf16_ema(*ptrs, 8, *hp, 1, None, 0.0, 0.001, None) == ERR_UNSUPPORTED
        assert lib.dvla_adamw_bf16_ema_guarded(*ptrs, 8, *hp, 0.1, p, w, 1, None) == ERR_UNSUPPORTED
    assert lib.dvla_adamw_bf16_ema(p, p, p, p, p, 8, *hp, 0, None, 0.0, 0.001, None) == ERR_ARG
    assert lib.dvla_adamw_bf16_ema(p, p, p, p, p, -1, *hp, 1, None, 0.0, 0.001, None) == ERR_ARG
    assert lib.dvla_adamw_bf16_ema(p, p, p, p, p, 0, *hp, 1, None, 0.0, 0.001, None) == 0
    assert lib.dvla_adamw_bf16_ema_guarded(p, p, p, p, p, 8, *hp, 0.1, None, w, 1, None) == ERR_ARG
    assert lib.dvla_adamw_bf16_ema_guarded(p, p, p, p, p, 8, *hp, 0.1, p, None, 1, None) == ERR_ARG
    assert lib.dvla_adamw_bf16_ema_guarded(p, p, p, p, p, 8, *hp, 0.1, p, w, 0, None) == ERR_ARG
    assert lib.dvla_adamw_bf16_ema_guarded(p, p, p, p, p, 8, *hp, 0.1, p, w, MAX_CAND + 1, None) == ERR_ARG
    assert lib.dvla_adamw_bf16_ema_guarded(p, p, p, p, p, 8, *hp, 0.1, p + 8, w, 1, None) == ERR_UNSUPPORTED
    assert lib.dvla_adamw_bf16_ema_guarded(p, p, p, p, p, 0, *hp, 0.1, p, w, 1, None) == 0
    # dvla_adamw_f32_master_ema(param, grad, m, v, shadow, ema, n, lr .. wd, step, grad_sumsq, max_norm, ema_w, stream)
    # dvla_adamw_f32_master_ema_guarded(param, grad, m, v, shadow, ema, n, lr .. wd, max_norm, state, ema_w, n_cand, stream)
    for k in (0, 1, 2, 3, 5):
        ptrs = [p] * 6
        ptrs[k] = None
        assert lib.dvla_adamw_f32_master_ema(*ptrs, 8, *hp, 1, None, 0.0, 0.001, None) == ERR_ARG
        assert lib.dvla_adamw_f32_master_ema_guarded(*ptrs, 8, *hp, 0.1, p, w, 1, None) == ERR_ARG
        ptrs[k] = p + 4
        assert lib.dvla_adamw_f32_master_ema(*ptrs, 8, *hp, 1, None, 0.0, 0.001, None) == ERR_UNSUPPORTED
        assert lib.dvla_adamw_f32_master_ema_guarded(*ptrs, 8, *hp, 0.1, p, w, 1, None) == ERR_UNSUPPORTED
    assert lib.dvla_adamw_f32_master_ema(p, p, p, p, p + 2, p, 8, *hp, 1, None, 0.0, 0.001, None) == ERR_UNSUPPORTED
    assert lib.dvla_adamw_f32_master_ema(p, p, p, p, None, p, 0, *hp, 1, None, 0.0, 0.001, None) == 0
    assert lib.dvla_adamw_f32_master_ema(p, p, p, p, p, p, 8, *hp, 0, None, 0.0, 0.001, None) == ERR_ARG
    assert lib.dvla_adamw_f32_master_ema_guarded(p, p, p, p, p, p, 8, *hp, 0.1, None, w, 1, None) == ERR_ARG
    assert lib.dvla_adamw_f32_master_ema_guarded(p, p, p, p, p, p, 8, *hp, 0.1, p, None, 1, None) == ERR_ARG
    assert lib.dvla_adamw_f32_master_ema_guarded(p, p, p, p, p, p, 8, *hp, 0.1, p, w, MAX_CAND + 1, None) == ERR_ARG
    assert lib.dvla_adamw_f32_master_ema_guarded(p, p, p, p, p, p, 8, *hp, 0.1, p + 8, w, 1, None) == ERR_UNSUPPORTED
    assert lib.dvla_adamw_f32_master_ema_guarded(p, p, p, p, None, p, 0, *hp, 0.1, p, w, 1, None) == 0
    # dvla_ema_swap_f32(param, ema, shadow, n, stream) / dvla_ema_swap_bf16(param, ema, stash, n, restore, stream)
    assert lib.dvla_ema_swap_f32(None, p, p, 8, None) == ERR_ARG
    assert lib.dvla_ema_swap_f32(p, None, p, 8, None) == ERR_ARG
    assert lib.dvla_ema_swap_f32(p, p, p, -1, None) == ERR_ARG
    assert lib.dvla_ema_swap_f32(p + 4, p, p, 8, None) == ERR_UNSUPPORTED
    assert lib.dvla_ema_swap_f32(p, p + 4, p, 8, None) == ERR_UNSUPPORTED
    assert lib.dvla_ema_swap_f32(p, p, p + 2, 8, None) == ERR_UNSUPPORTED
    assert lib.dvla_ema_swap_f32(p, p, None, 0, None) == 0
    for k in range(3):
        ptrs = [p] * 3
        ptrs[k] = None
        assert lib.dvla_ema_swap_bf16(*ptrs, 8, 0, None) == ERR_ARG
        ptrs[k] = p + (4 if k == 1 else 2)
        assert lib.dvla_ema_swap_bf16(*ptrs, 8, 1, None) == ERR_UNSUPPORTED
    assert lib.dvla_ema_swap_bf16(p, p, p, -1, 0, None) == ERR_ARG
    assert lib.dvla_ema_swap_bf16(p, p, p, 0, 0, None) == 0
    del keep


@pytest.mark.parametrize("bad", [1.0, 0.0, -0.1, 1.5, float("nan")])
def test_constructor_rejects_a_decay_outside_the_open_unit_interval_before_it_touches_the_reducer(bad):
    from dreamvla_amd.optim import FlatAdamW
    with pytest.raises(ValueError, match="ema_decay"):
        FlatAdamW(None, ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        FlatAdamW(None, ema_decay=bad, skip_nonfinite=True)
