"""CPU: parameter groups of FlatAdamW -- the C surface (symbols, dvla_group_scalars), the group-map builder, the validation of
the groups and weight_decay_groups.  Everything that is a float is compared as its bits."""
import ctypes as C
import os
import re
import struct

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = (0.9, 0.999)


def _f32_bits(x):
    """the bits of the double x rounded to float (RNE, struct's conversion), as the C cast gives them"""
    return struct.unpack("<I", struct.pack("<f", x))[0]


_bits = _f32_bits       # of a value that is a float already: its bits


def test_symbols_are_bound_and_the_abi_is_still_9():
    from dreamvla_amd import _lib
    for name in ("dvla_group_scalars", "dvla_adamw_bf16_grouped", "dvla_adamw_f32_master_grouped"):
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.load(), name)
    assert _lib.ABI_VERSION == 9 and _lib.load().dvla_abi_version() == 9
    txt = open(os.path.join(ROOT, "include", "dvla.h")).read()
    assert re.search(r"#define\s+DVLA_ABI_VERSION\s+9\b", txt)
    assert int(re.search(r"#define\s+DVLA_STEP_MAX_GROUPS\s+(\d+)", txt).group(1)) == _lib.STEP_MAX_GROUPS == 64
    # the mirror of dvla_group_row: three floats and one step size per candidate count
    assert C.sizeof(_lib.GroupRow) == 4 * (3 + _lib.STEP_MAX_CANDIDATES)
    body = re.search(r"typedef struct dvla_group_row \{(.*?)\} dvla_group_row;", txt).group(1)
    assert [f[0] for f in _lib.GroupRow._fields_] == re.findall(r"([a-z_0-9]+)\s*(?:\[\w+\])?\s*[,;]", body)


GROUPS = {2: ([1e-3, 2.5e-4], [1e-2, 0.0]),
          3: ([1e-3, 0.0, 3.7e-5], [0.05, 0.1, 0.0])}       # an lr of 0, a weight decay of 0


@pytest.mark.parametrize("n_cand", [1, 9])
@pytest.mark.parametrize("base", [1, 1000])
@pytest.mark.parametrize("n_groups", [2, 3])
def test_group_scalars_are_the_one_group_entry_points_floats(n_groups, base, n_cand):
    from dreamvla_amd import _lib
    lib = _lib.load()
    lrs, wds = GROUPS[n_groups]
    rows = (_lib.GroupRow * n_groups)()
    assert lib.dvla_group_scalars((C.c_double * n_groups)(*lrs), (C.c_double * n_groups)(*wds), n_groups, BETAS[0], BETAS[1], base,
                                  n_cand, rows) == 0
    cand = (_lib.StepScalars * _lib.STEP_MAX_CANDIDATES)()
    for g, (lr, wd) in enumerate(zip(lrs, wds)):
        # the float64 restatement: Python floats are doubles, the expressions are those of dvla.h
        assert _bits(rows[g].decay) == _f32_bits(1.0 - lr * wd), g
        assert _bits(rows[g].lr) == _f32_bits(lr) and _bits(rows[g].weight_decay) == _f32_bits(wd), g
        assert lib.dvla_step_candidates(lr, BETAS[0], BETAS[1], base, n_cand, cand) == 0
        for j in range(_lib.STEP_MAX_CANDIDATES):
            t = base + min(j, n_cand - 1)           # rows past n_cand repeat the last
            assert _bits(rows[g].step_size[j]) == _f32_bits((lr / (1.0 - BETAS[0] ** t)) * -1.0), (g, j)
            # and what the guarded one-group step runs on for this lr
            assert _bits(rows[g].step_size[j]) == _bits(cand[min(j, n_cand - 1)].step_size), (g, j)


def test_group_scalars_refuse_bad_arguments():
    from dreamvla_amd import _lib
    lib = _lib.load()
    one = (C.c_double * 65)(*([1e-3] * 65))
    rows = (_lib.GroupRow * 65)()
    assert lib.dvla_group_scalars(one, one, 64, 0.9, 0.999, 1, 1, rows) == 0
    for n_groups, base, n_cand in ((0, 1, 1), (65, 1, 1), (2, 0, 1), (2, 1, 0), (2, 1, 10)):
        assert lib.dvla_group_scalars(one, one, n_groups, 0.9, 0.999, base, n_cand, rows) == -1, (n_groups, base, n_cand)
    assert lib.dvla_group_scalars(None, one, 2, 0.9, 0.999, 1, 1, rows) == -1


# ---- the map builder ----------------------------------------------------------------------------------------------------------
def _map(offsets, sizes, total, gids, stepped, n_groups):
    from dreamvla_amd.optim import build_group_map
    m = build_group_map(offsets, sizes, total, gids, stepped, n_groups)
    assert m.dtype == torch.uint8 and m.device.type == "cpu" and m.numel() == -(-total // 8)
    return m.tolist()


def test_map_group_boundary_on_a_multiple_of_8():
    assert _map([0, 16], [16, 24], 40, [0, 1], [True, True], 2) == [0, 0, 1, 1, 1]


def test_map_parameter_of_5_elements_alone_in_its_vector_and_a_tail_parameter_of_3():
    # 12 elements (vectors 0-1, the second partial), 5 elements alone in vector 2, 9 elements (vectors 3-4), 3 elements that are
    # all ragged tail: 35 = 8 * 4 + 3, so the last byte stands for the tail
    got = _map([0, 16, 24, 40], [12, 5, 9, 3], 43, [0, 1, 0, 2], [True] * 4, 3)
    assert got == [0, 0, 1, 0, 0, 2]


def test_map_unstepped_parameter_in_the_middle_and_gaps_are_255():
    # parameter 1 (vectors 2-3) is not stepped; parameters are padded to 32 elements here (the reducer pads to 128): the
    # vectors of the gaps are nobody's
    got = _map([0, 32, 64], [10, 16, 17], 81, [0, 1, 1], [True, False, True], 2)
    assert got == [0, 0, 255, 255, 255, 255, 255, 255, 1, 1, 1]
    assert _map([0, 8], [8, 8], 16, [0, 1], [False, False], 2) == [255, 255]


def test_map_of_the_gpu_tests_layout():
    # tests/test_param_groups_gpu.py, bucket 0: [(1300,), (5,), (1711,), (3,)] in groups 0, 1, 0, 1, parameters on multiples of 8
    got = _map([0, 1304, 1312, 3024], [1300, 5, 1711, 3], 3027, [0, 1, 0, 1], [True] * 4, 2)
    assert len(got) == 379 and got[:163] == [0] * 163 and got[163] == 1 and got[164:378] == [0] * 214 and got[378] == 1


def test_map_refuses_a_bad_offset_or_group_id():
    from dreamvla_amd.optim import build_group_map
    with pytest.raises(ValueError, match="multiple of 8"):
        build_group_map([0, 12], [12, 4], 16, [0, 1], [True, True], 2)
    with pytest.raises(ValueError, match="group id"):
        build_group_map([0], [8], 8, [2], [True], 2)
    with pytest.raises(ValueError, match="ends at"):
        build_group_map([0], [9], 8, [0], [True], 1)


# ---- validation of the groups ---------------------------------------------------------------------------------------------------
DEFAULTS = dict(lr=1e-3, betas=BETAS, eps=1e-8, weight_decay=1e-2)


def _ps(n=4):
    return [torch.nn.Parameter(torch.zeros(i + 1, 3)) for i in range(n)]


def test_groups_that_partition_the_parameters_are_accepted_in_any_order():
    from dreamvla_amd.optim import resolve_param_groups
    ps = _ps()
    given = [{"params": [ps[3], ps[0]], "lr": 1e-4}, {"params": [ps[2], ps[1]], "weight_decay": 0.0}]
    got = resolve_param_groups(ps, given, DEFAULTS)
    assert [[id(p) for p in g["params"]] for g in got] == [[id(ps[3]), id(ps[0])], [id(ps[2]), id(ps[1])]]
    assert got[0]["lr"] == 1e-4 and "weight_decay" not in got[0] and got[1]["weight_decay"] == 0.0
    assert given[0]["params"] == [ps[3], ps[0]] and got[0] is not given[0]          # the caller's dicts are left alone
    # a group may restate the common betas / eps
    resolve_param_groups(ps, [{"params": ps, "betas": [0.9, 0.999], "eps": 1e-8}], DEFAULTS)


def test_each_bad_grouping_raises_value_error_naming_the_parameter():
    from dreamvla_amd.optim import resolve_param_groups
    ps = _ps()
    with pytest.raises(ValueError, match=r"parameter 2 of reducer.params \(shape \(3, 3\)\) is in no group"):
        resolve_param_groups(ps, [{"params": [ps[0], ps[1]]}, {"params": [ps[3]]}], DEFAULTS)
    with pytest.raises(ValueError, match=r"parameter 1 of reducer.params \(shape \(2, 3\)\) is in two groups \(0 and 1\)"):
        resolve_param_groups(ps, [{"params": [ps[0], ps[1]]}, {"params": [ps[1], ps[2], ps[3]]}], DEFAULTS)
    with pytest.raises(ValueError, match=r"parameter 0 of reducer.params .* is in two groups \(0 and 0\)"):
        resolve_param_groups(ps, [{"params": [ps[0], ps[0], ps[1], ps[2], ps[3]]}], DEFAULTS)
    stranger = torch.nn.Parameter(torch.zeros(7))
    with pytest.raises(ValueError, match=r"parameter 1 of group 1 \(shape \(7,\)\) is not a parameter of the reducer"):
        resolve_param_groups(ps, [{"params": ps[:2]}, {"params": [ps[2], stranger, ps[3]]}], DEFAULTS)
    with pytest.raises(ValueError, match="at most 64 parameter groups"):
        many = _ps(65)
        resolve_param_groups(many, [{"params": [p]} for p in many], DEFAULTS)
    with pytest.raises(ValueError, match="group 1 has betas"):
        resolve_param_groups(ps, [{"params": ps[:2]}, {"params": ps[2:], "betas": (0.9, 0.95)}], DEFAULTS)
    with pytest.raises(ValueError, match="group 0 has eps"):
        resolve_param_groups(ps, [{"params": ps[:2], "eps": 1e-6}, {"params": ps[2:]}], DEFAULTS)
    with pytest.raises(ValueError, match="non-empty list"):
        resolve_param_groups(ps, [], DEFAULTS)


def test_sixty_four_groups_are_accepted():
    from dreamvla_amd.optim import resolve_param_groups
    ps = _ps(64)
    assert len(resolve_param_groups(ps, [{"params": [p]} for p in ps], DEFAULTS)) == 64


def test_betas_or_eps_edited_after_construction_are_caught():
    from dreamvla_amd.optim import common_betas_eps
    groups = [dict(DEFAULTS), dict(DEFAULTS, lr=1e-5), dict(DEFAULTS, betas=[0.9, 0.999])]
    assert common_betas_eps(groups) == (0.9, 0.999, 1e-8)
    groups[1]["eps"] = 1e-6
    with pytest.raises(ValueError, match="group 1 has"):
        common_betas_eps(groups)
    groups[1]["eps"] = 1e-8
    groups[2]["betas"] = (0.9, 0.95)
    with pytest.raises(ValueError, match="group 2 has"):
        common_betas_eps(groups)


# ---- weight_decay_groups --------------------------------------------------------------------------------------------------------
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.pos_embed = torch.nn.Parameter(torch.zeros(1, 5, 8))         # 3-D: only `skip` keeps it from being decayed
        self.scale = torch.nn.Parameter(torch.zeros(1, 8))                # 2-D and not skipped: decayed
        self.fc = torch.nn.Linear(8, 4)
        self.norm = torch.nn.LayerNorm(4)
        self.frozen = torch.nn.Linear(4, 4)
        self.frozen.weight.requires_grad_(False)                          # left out; its bias stays trainable


def test_weight_decay_groups_membership_written_out_by_hand():
    from dreamvla_amd.optim import weight_decay_groups
    m = _Tiny()
    groups = weight_decay_groups(m, 0.05, skip=("pos_embed",))
    assert [sorted(g) for g in groups] == [["params", "weight_decay"]] * 2
    assert [g["weight_decay"] for g in groups] == [0.0, 0.05]
    plain, decayed = ([id(p) for p in g["params"]] for g in groups)
    assert plain == [id(m.pos_embed), id(m.fc.bias), id(m.norm.weight), id(m.norm.bias), id(m.frozen.bias)]
    assert decayed == [id(m.scale), id(m.fc.weight)]
    # the same from named parameters; without `skip` the 3-D pos_embed is decayed
    groups = weight_decay_groups(list(m.named_parameters()), 0.05)
    assert [id(p) for p in groups[1]["params"]] == [id(m.pos_embed), id(m.scale), id(m.fc.weight)]
    # plain torch groups: torch.optim.AdamW takes them
    opt = torch.optim.AdamW(weight_decay_groups(m, 0.05, skip=("pos_embed",)), lr=1e-3)
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 0.05]
    # a group that would be empty is omitted
    only = weight_decay_groups(torch.nn.LayerNorm(4), 0.05)
    assert len(only) == 1 and only[0]["weight_decay"] == 0.0 and len(only[0]["params"]) == 2
