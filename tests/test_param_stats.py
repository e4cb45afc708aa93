"""CPU: the host side of FlatAdamW.parameter_stats() -- the chunk table (optim.build_chunk_table), optim.stats_by_module, the
argument checks of the dvla_segment_* entry points that return before anything touches a device, and the validation of `what`."""
import os
import types

import pytest
import torch

from dreamvla_amd import _lib
from dreamvla_amd.optim import FlatAdamW, build_chunk_table, stats_by_module

CHUNK = _lib.STATS_CHUNK
SIZES = [0, 1, 7, 8, 9, 127, 128, 129, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def _layout(sizes, align, lead=0):
    """offsets of parameters of `sizes` elements, each padded to `align` elements, the first at element `lead` -> (offsets, total)"""
    offsets, off = [], lead
    for n in sizes:
        offsets.append(off)
        off += -(-n // align) * align
    return offsets, off


# 128: the reducer's padding (gaps behind most sizes); 8: the tightest layout the kernels take; a permutation; and the same
# sizes pushed 5 * 128 elements up, as if other parameters sat in front
LAYOUTS = {"reducer": (SIZES, 128, 0), "tight": (SIZES, 8, 0), "reversed": (SIZES[::-1], 128, 0), "shifted": (SIZES, 128, 640),
           "wide_gaps": (SIZES, 1024, 8)}


def test_chunk_is_published_and_a_multiple_of_8():
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dvla.h")).read()
    assert f"#define DVLA_STATS_CHUNK {CHUNK}\n" in txt and f"#define DVLA_STATS_PARTIAL_BYTES {_lib.STATS_PARTIAL_BYTES}\n" in txt
    assert CHUNK % 8 == 0 and CHUNK % (256 * 8) == 0


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_every_element_is_in_exactly_one_chunk_and_no_gap_element_in_any(name):
    sizes, align, lead = LAYOUTS[name]
    offsets, total = _layout(sizes, align, lead)
    total += 3                                       # and a few elements behind the last parameter
    chunks, segs = build_chunk_table(offsets, sizes, total)
    assert chunks.dtype == segs.dtype == torch.int64 and chunks.shape[1] == 2 and segs.shape == (len(sizes), 3)
    cover = torch.zeros(total, dtype=torch.int64)
    owner = torch.full((total,), -1, dtype=torch.int64)
    for j, (off, n) in enumerate(zip(offsets, sizes)):
        owner[off:off + n] = j
    for j, (first, cnt, out) in enumerate(segs.tolist()):
        assert out == j and cnt == -(-sizes[j] // CHUNK)
        rows = chunks[first:first + cnt].tolist()
        assert sum(ln for _, ln in rows) == sizes[j]
        at = offsets[j]
        for start, ln in rows:                       # consecutive, in order, each inside parameter j
            assert start == at and start % 8 == 0 and 0 < ln <= CHUNK
            assert bool((owner[start:start + ln] == j).all())
            cover[start:start + ln] += 1
            at += ln
    assert int(segs[:, 1].sum()) == chunks.shape[0]                  # no chunk belongs to nobody
    assert bool((cover[owner >= 0] == 1).all()) and bool((cover[owner < 0] == 0).all())
    assert int((owner < 0).sum()) > 0                                # the layout did have gaps


def test_cuts_are_relative_to_the_parameters_own_start():
    """the same sizes at other offsets, in another order, beside other neighbours: the same cuts, counted from each parameter's
    first element"""
    def cuts(name):
        sizes, align, lead = LAYOUTS[name]
        offsets, total = _layout(sizes, align, lead)
        chunks, segs = build_chunk_table(offsets, sizes, total)
        return {n: [(s - off, ln) for s, ln in chunks[f:f + c].tolist()] for n, off, (f, c, _) in zip(sizes, offsets, segs.tolist())}
    want = cuts("reducer")
    assert want[3 * CHUNK + 5] == [(0, CHUNK), (CHUNK, CHUNK), (2 * CHUNK, CHUNK), (3 * CHUNK, 5)]
    assert want[CHUNK + 1] == [(0, CHUNK), (CHUNK, 1)] and want[CHUNK] == [(0, CHUNK)] and want[0] == [] and want[9] == [(0, 9)]
    for name in LAYOUTS:
        assert cuts(name) == want, name


def test_the_table_does_not_depend_on_what_the_step_leaves_alone_and_takes_the_output_indices():
    """every parameter is in the table -- one that receives no gradient reports zeros because its buffers hold zeros --, and the
    third column is where its results go"""
    sizes = [300, 0, CHUNK + 9]
    offsets, total = _layout(sizes, 128)
    chunks, segs = build_chunk_table(offsets, sizes, total, out_index=[7, 2, 5])
    assert segs.tolist() == [[0, 1, 7], [1, 0, 2], [1, 2, 5]]
    assert chunks.tolist() == [[0, 300], [384, CHUNK], [384 + CHUNK, 9]]
    # the buckets of one optimizer write consecutive regions of one scratch: a later bucket's records start at first_record
    chunks2, segs2 = build_chunk_table(offsets, sizes, total, out_index=[7, 2, 5], first_record=40)
    assert torch.equal(chunks2, chunks) and segs2.tolist() == [[40, 1, 7], [41, 0, 2], [41, 2, 5]]
    empty = build_chunk_table([], [], 0)
    assert empty[0].shape == (0, 2) and empty[1].shape == (0, 3)


def test_the_builder_refuses_a_layout_the_kernels_cannot_take():
    with pytest.raises(ValueError, match="multiple of 8"):
        build_chunk_table([0, 12], [8, 8], 64)
    with pytest.raises(ValueError, match="ends at element"):
        build_chunk_table([0, 8], [8, 57], 64)
    with pytest.raises(ValueError, match="chunk length"):
        build_chunk_table([0], [8], 8, chunk=100)


# ---- stats_by_module -----------------------------------------------------------------------------------------------------------
def _named():
    ps = [torch.nn.Parameter(torch.zeros(1)) for _ in range(7)]
    names = ["trunk.h.0.attn.weight", "trunk.h.0.attn.bias", "trunk.h.1.mlp.weight", "trunk.ln_f.weight", "heads.arm.fc.weight",
             "heads.gripper.weight"]
    named = list(zip(names, ps[:6])) + [("heads.tied.weight", ps[4])]        # ps[4] shared under a second name; ps[6] unnamed
    red = types.SimpleNamespace(params=[ps[5], ps[6], ps[0], ps[1], ps[2], ps[3], ps[4]])
    stats = {"grad_norm": torch.tensor([3.0, 1.0, 4.0, 12.0, 3.0, 2.0, 5.0]),
             "grad_absmax": torch.tensor([0.5, 9.0, 0.25, float("inf"), 2.0, 1.0, 4.0]),
             "grad_nonfinite": torch.tensor([0, 2, 0, 1, 0, 0, 3])}
    return named, red, stats


def test_stats_by_module_on_hand_made_names():
    named, red, stats = _named()
    names, out = stats_by_module(stats, named, red, depth=1)
    assert names == ["heads", "<unnamed>", "trunk"]
    assert out["grad_norm"].tolist() == pytest.approx([(9 + 25) ** 0.5, 1.0, (16 + 144 + 9 + 4) ** 0.5], rel=1e-6)
    assert out["grad_absmax"].tolist() == [4.0, 9.0, float("inf")] and out["grad_nonfinite"].tolist() == [3, 2, 1]
    assert out["grad_nonfinite"].dtype == torch.int64 and out["grad_norm"].dtype == torch.float32
    names, out = stats_by_module(stats, named, red, depth=2)
    assert names == ["heads.gripper", "<unnamed>", "trunk.h", "trunk.ln_f", "heads.arm"]      # the shared one under its first name
    assert out["grad_norm"].tolist() == pytest.approx([3.0, 1.0, 13.0, 2.0, 5.0], rel=1e-6)
    assert out["grad_absmax"].tolist() == [0.5, 9.0, float("inf"), 1.0, 4.0] and out["grad_nonfinite"].tolist() == [0, 2, 1, 0, 3]
    names, out = stats_by_module(stats, named, red, depth=3)
    assert names == ["heads.gripper.weight", "<unnamed>", "trunk.h.0", "trunk.h.1", "trunk.ln_f.weight", "heads.arm.fc"]
    assert out["grad_norm"].tolist() == pytest.approx([3.0, 1.0, (16 + 144) ** 0.5, 3.0, 2.0, 5.0], rel=1e-6)
    assert out["grad_nonfinite"].tolist() == [0, 2, 1, 0, 0, 3]


def test_stats_by_module_takes_a_module_and_refuses_what_it_cannot_combine():
    model = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 2))
    red = types.SimpleNamespace(params=list(model.parameters()))
    names, out = stats_by_module({"param_norm": torch.tensor([1.0, 2.0, 2.0, 4.0])}, model, red, depth=1)
    assert names == ["0", "1"] and out["param_norm"].tolist() == pytest.approx([5 ** 0.5, 20 ** 0.5], rel=1e-6)
    with pytest.raises(ValueError, match="shape"):
        stats_by_module({"param_norm": torch.ones(3)}, model, red)
    with pytest.raises(ValueError, match="combine"):
        stats_by_module({"param_mean": torch.ones(4)}, model, red)


# ---- the C entry points' argument checks (nothing here reaches a device) -------------------------------------------------------
def test_c_entry_points_check_their_arguments_before_touching_the_device():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    p = 4096          # never dereferenced: every call below returns from its argument checks

    def stats(fn, x=p, n=64, chunks=p, n_chunks=1, part=p):
        return fn(x, n, chunks, n_chunks, part, None)

    def adam(fn, m=p, v=p, n=64, chunks=p, n_chunks=1, part=p, step=1):
        return fn(m, v, n, chunks, n_chunks, part, 0.999, 1e-8, step, None)

    def combine(part=p, n_chunks=1, segs=p, n_segs=1, sumsq=p, absmax=p, bad=p, n_out=1):
        return lib.dvla_segment_combine(part, n_chunks, segs, n_segs, sumsq, absmax, bad, n_out, None)

    for fn in (lib.dvla_segment_stats_bf16, lib.dvla_segment_stats_f32):
        for name in ("x", "chunks", "part"):
            assert stats(fn, **{name: None}) == ERR_ARG, name
        for name in ("n", "n_chunks"):
            assert stats(fn, **{name: -1}) == ERR_ARG, name
        assert stats(fn, n_chunks=0) == 0 and stats(fn, n_chunks=0, x=p + 2) == 0          # a bucket with no segments: nothing launched
        assert stats(fn, x=p + 4) == ERR_UNSUPPORTED and stats(fn, part=p + 8) == ERR_UNSUPPORTED
    for fn in (lib.dvla_segment_adam_bf16, lib.dvla_segment_adam_f32):
        for name in ("m", "v", "chunks", "part"):
            assert adam(fn, **{name: None}) == ERR_ARG, name
        for name in ("n", "n_chunks"):
            assert adam(fn, **{name: -1}) == ERR_ARG, name
        assert adam(fn, step=0) == ERR_ARG
        assert adam(fn, n_chunks=0) == 0
        assert adam(fn, m=p + 4) == ERR_UNSUPPORTED and adam(fn, v=p + 8) == ERR_UNSUPPORTED
    for name in ("part", "segs", "sumsq"):                      # (absmax and nonfinite may be null: the Adam term has neither)
        assert combine(**{name: None}) == ERR_ARG, name
    for name in ("n_chunks", "n_segs", "n_out"):
        assert combine(**{name: -1}) == ERR_ARG, name
    assert combine(n_segs=0) == 0 and combine(n_segs=0, absmax=None, bad=None) == 0 and combine(part=p + 8) == ERR_UNSUPPORTED


# ---- `what` --------------------------------------------------------------------------------------------------------------------
def test_an_unknown_entry_of_what_raises_before_anything_else():
    stub = types.SimpleNamespace(_ema_active=False)            # validation comes first: no buffer, no library is reached
    for bad in (("grad", "moments"), "updates", ("",)):
        with pytest.raises(ValueError, match="unknown entry"):
            FlatAdamW.parameter_stats(stub, what=bad)
    with pytest.raises(RuntimeError, match="ema_weights"):
        FlatAdamW.parameter_stats(types.SimpleNamespace(_ema_active=True), what=("grad",))
