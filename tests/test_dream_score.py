"""CPU: scoring the dreams -- the float64 restatement of the metrics (tests/dream_score_ref.py) against
closed forms, the two new C-ABI entry points, the argument rules of ops.image_quality / ops.depth_quality, and the host rules of
RolloutEngine(score_dreams=True): constructor checks, which rows are valid over steps and resets, which pairs are scored."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import dream_score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
def test_window_is_normalised_and_symmetric():
    w = R.gaussian_window()
    assert w.shape == (11,) and abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1]) and w.argmax() == 5
    assert abs(w[4] / w[5] - np.exp(-1 / 4.5)) < 1e-15


def test_ssim_of_an_image_with_itself_is_one():
    a = _rand_u8((19, 23, 3), 1)
    assert abs(R.ssim(a, a) - 1) < 1e-12
    q = R.image_quality(a[None], a[None])
    assert q["sse"][0] == 0 and q["mse"][0] == 0 and q["psnr"][0] == np.inf


def test_ssim_black_against_white():
    a, b = np.zeros((15, 13, 3), np.uint8), np.full((15, 13, 3), 255, np.uint8)
    assert abs(R.ssim(a, b) - R.C1 / (255.0 ** 2 + R.C1)) < 1e-12
    q = R.image_quality(a[None], b[None])
    assert q["sse"][0] == 15 * 13 * 3 * 255 ** 2 and abs(q["psnr"][0]) < 1e-12


def test_ssim_is_symmetric():
    a, b = _rand_u8((17, 21, 3), 2), _rand_u8((17, 21, 3), 3)
    assert R.ssim(a, b) == pytest.approx(R.ssim(b, a), abs=1e-15)


def test_the_11_x_11_image_has_one_window():
    a, b = _rand_u8((11, 11, 3), 4), _rand_u8((11, 11, 3), 5)
    w2 = np.outer(R.gaussian_window(), R.gaussian_window())
    want = []
    for c in range(3):
        x, y = a[..., c].astype(np.float64), b[..., c].astype(np.float64)
        assert R.ssim_map(x, y).shape == (1, 1)
        ux, uy = (w2 * x).sum(), (w2 * y).sum()
        vx, vy, vxy = (w2 * (x - ux) ** 2).sum(), (w2 * (y - uy) ** 2).sum(), (w2 * (x - ux) * (y - uy)).sum()
        want.append((2 * ux * uy + R.C1) * (2 * vxy + R.C2) / ((ux * ux + uy * uy + R.C1) * (vx + vy + R.C2)))
    assert R.ssim(a, b) == pytest.approx(np.mean(want), abs=1e-12)


def test_ssim_restatement_vs_skimage():
    sk = pytest.importorskip("skimage.metrics")
    for shape, seed in (((11, 11, 3), 6), ((43, 75, 3), 7)):
        a, b = _rand_u8(shape, seed), _rand_u8(shape, seed + 100)
        want = sk.structural_similarity(a, b, gaussian_weights=True, use_sample_covariance=False, data_range=255, channel_axis=-1)
        assert abs(R.ssim(a, b) - want) <= 1e-12


def test_depth_metrics_of_a_perfect_prediction():
    t = np.random.default_rng(8).uniform(0.1, 5.0, size=(2, 13, 9)).astype(np.float32)
    t[1, :4] = 0.0
    q = R.depth_quality(t, t)
    assert q["valid"].tolist() == [13 * 9, 9 * 9]
    assert np.all(q["abs_rel"] == 0) and np.all(q["rmse"] == 0) and np.all(q["silog"] == 0) and np.all(q["delta1"] == 1)


def test_depth_metrics_closed_form_and_empty_map():
    t = np.full((2, 4, 5), 2.0, np.float32)
    p = np.full((2, 4, 5), 3.0, np.float32)
    p[0, 0, 0] = -1.0                                  # clamped to 0: |0 - 2| / 2 = 1, ratio inf
    t[1] = 0.0                                         # nothing valid
    q = R.depth_quality(p, t)
    assert q["valid"].tolist() == [20, 0] and q["delta1_count"].tolist() == [0, 0]
    assert q["abs_rel"][0] == pytest.approx((19 * 0.5 + 1.0) / 20) and q["rmse"][0] == pytest.approx(np.sqrt((19 * 1.0 + 4.0) / 20))
    assert all(np.isnan(q[k][1]) for k in ("abs_rel", "rmse", "silog", "delta1"))


# ---------------------------------------------------------------------------------------------------
# library surface
# ---------------------------------------------------------------------------------------------------
def _header():
    txt = open(os.path.join(ROOT, "include", "dvla.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


C_TYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int}


@pytest.mark.parametrize("symbol", ["dvla_image_quality", "dvla_depth_quality", "dvla_image_quality_partial_len",
                                    "dvla_depth_quality_partial_len"])
def test_entry_points_are_exported_and_bound_as_declared(symbol):
    from dreamvla_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, symbol)
    assert lib.dvla_abi_version() == 9 == _lib.ABI_VERSION                  # the version include/dvla.h declares
    ret, decl = re.search(r"(int64_t|int)\s+%s\s*\((.*?)\)\s*;" % symbol, _header(), flags=re.S).groups()
    want = []
    for arg in decl.split(","):
        typ = re.sub(r"\s*\b[A-Za-z_][A-Za-z0-9_]*\s*$", "", " ".join(arg.split()))       # drop the parameter name
        want.append(ctypes.c_void_p if typ.endswith("*") else C_TYPES[typ])
    res, args = _lib.SYMBOLS[symbol]
    assert res is C_TYPES[ret] and list(args) == want


def test_partial_len_needs_no_gpu():
    from dreamvla_amd import _lib
    lib = _lib.load()
    assert lib.dvla_image_quality_partial_len(3, 224, 224) == 2 * 3 * 7 * 7      # 32 x 32 tiles of the 214 x 214 map, two words each
    assert lib.dvla_image_quality_partial_len(1, 11, 43) == 2 * 1 * 2
    assert lib.dvla_image_quality_partial_len(5, 10, 224) == 0 and lib.dvla_image_quality_partial_len(-1, 224, 224) == 0
    assert lib.dvla_depth_quality_partial_len(2, 224, 224) == 6 * 2 * 13 and lib.dvla_depth_quality_partial_len(1, 13, 9) == 6


def test_entry_points_check_their_arguments_before_any_launch():
    from dreamvla_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    assert lib.dvla_image_quality(None, p, 1, 11, 11, p, p, p, None) == -1
    assert lib.dvla_image_quality(p, p, -1, 11, 11, p, p, p, None) == -1
    assert lib.dvla_image_quality(p, p, 1, 10, 11, p, p, p, None) == -3
    assert lib.dvla_image_quality(p, p, 1, 11, 10, p, p, p, None) == -3
    assert lib.dvla_image_quality(p, p, 0, 11, 11, p, p, p, None) == 0
    assert lib.dvla_depth_quality(p, None, 1, 4, 4, p, p, p, None) == -1
    assert lib.dvla_depth_quality(p, p, -2, 4, 4, p, p, p, None) == -1
    assert lib.dvla_depth_quality(p, p, 0, 4, 4, p, p, p, None) == 0


# ---------------------------------------------------------------------------------------------------
# argument rules
# ---------------------------------------------------------------------------------------------------
def test_image_quality_argument_rules():
    from dreamvla_amd import ops
    from dreamvla_amd._lib import DvlaError
    a = torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(DvlaError):                            # no CPU fallback
        ops.image_quality(a, a)
    with pytest.raises(ValueError):
        ops.image_quality(a.float(), a.float())               # dtype
    with pytest.raises(ValueError):
        ops.image_quality(a, a.float())
    with pytest.raises(ValueError):
        ops.image_quality(a[0, 0], a[0, 0])                   # rank
    with pytest.raises(ValueError):
        ops.image_quality(a, a[:1])                           # mismatch
    with pytest.raises(ValueError):
        ops.image_quality(a[..., :2], a[..., :2])             # not RGB
    with pytest.raises(ValueError):
        ops.image_quality(a[:, :10], a[:, :10])               # h < 11
    with pytest.raises(ValueError):
        ops.image_quality(a[:, :, :10], a[:, :, :10])         # w < 11


def test_depth_quality_argument_rules():
    from dreamvla_amd import ops
    from dreamvla_amd._lib import DvlaError
    p = torch.zeros(2, 13, 9)
    with pytest.raises(DvlaError):
        ops.depth_quality(p, p)
    with pytest.raises(ValueError):
        ops.depth_quality(p.double(), p.double())
    with pytest.raises(ValueError):
        ops.depth_quality(p, p.to(torch.bfloat16))
    with pytest.raises(ValueError):
        ops.depth_quality(p[0, 0], p[0, 0])
    with pytest.raises(ValueError):
        ops.depth_quality(p, p[:, :12])


# ---------------------------------------------------------------------------------------------------
# engine host rules (a stand-in model, CPU tensors, the metric kernels replaced by the restatement)
# ---------------------------------------------------------------------------------------------------
def _stub(**heads):
    from tests.test_rollout_host_rules import _FakeDiTModel
    m = _FakeDiTModel()
    for k, v in heads.items():
        setattr(m, k, v)
    return m


def test_engine_constructor_checks():
    from dreamvla_amd.rollout import RolloutEngine
    m = _stub(obs_pred=True, depth_pred=True, sam_feat_pred=True)
    plain = RolloutEngine(m, 2, use_graph=False, dreams=("image",))
    assert plain.score_dreams is False and plain.horizon == 3 and plain.last_dream_scores == {} and plain._dream_ring is None
    eng = RolloutEngine(m, 2, use_graph=False, dreams=("image", "depth", "sam"), score_dreams=True)
    assert eng.score_dreams and eng.horizon == 3 and eng._scored == ("image", "depth")
    assert RolloutEngine(m, 2, use_graph=False, dreams=("depth",), score_dreams=True, horizon=5).horizon == 5
    with pytest.raises(ValueError):
        RolloutEngine(m, 2, use_graph=False, score_dreams=True)                               # no dreams at all
    with pytest.raises(ValueError):
        RolloutEngine(m, 2, use_graph=False, dreams=("sam",), score_dreams=True)              # nothing that has a target
    with pytest.raises(ValueError):
        RolloutEngine(m, 2, use_graph=False, dreams=("image",), sample="all", score_dreams=True)
    with pytest.raises(ValueError):
        RolloutEngine(m, 2, use_graph=False, dreams=("image",), score_dreams=True, horizon=0)
    m.pred_num = 2
    with pytest.raises(ValueError):
        RolloutEngine(m, 2, use_graph=False, dreams=("image",), score_dreams=True)
    RolloutEngine(m, 2, use_graph=False, dreams=("image",))                                   # not scoring: pred_num is no concern


def test_engine_step_without_frames_raises():
    from dreamvla_amd.rollout import RolloutEngine
    m = _stub(obs_pred=True, depth_pred=True)
    eng = RolloutEngine(m, 2, use_graph=False, dreams=("image",), score_dreams=True)
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError, match="frames_u8"):
        eng.step(x, x, torch.zeros(2, 7), torch.zeros(2, 77, dtype=torch.long))
    assert eng.tokens is None and int(eng.since_reset.sum()) == 0                             # refused before anything was pushed


def _ref_image_quality(a, b):
    lead = tuple(a.shape[:-3])
    q = R.image_quality(a.reshape(-1, *a.shape[-3:]).numpy(), b.reshape(-1, *b.shape[-3:]).numpy())
    return {k: torch.from_numpy(np.asarray(v)).to(torch.int64 if k == "sse" else torch.float32).view(lead) for k, v in q.items()}


def _ref_depth_quality(p, t):
    lead = tuple(p.shape[:-2])
    q = R.depth_quality(p.reshape(-1, *p.shape[-2:]).numpy(), t.reshape(-1, *t.shape[-2:]).numpy())
    q.pop("delta1_count")
    return {k: torch.from_numpy(np.asarray(v)).to(torch.int64 if k == "valid" else torch.float32).view(lead) for k, v in q.items()}


def test_engine_valid_rows_and_scored_pairs(monkeypatch):
    """11 control steps of 3 episodes, horizon 3: episode 2 is reset during the first `horizon` steps (before step 1), episode 1 in
    mid-run (before step 6).  `valid` against a per-episode restatement; the valid rows are the (dream of t - 3, frame of t) and
    (frame of t - 3, frame of t) pairs; the others hold NaN / -1; a step without depth_now has no depth entry."""
    from dreamvla_amd import ops
    from dreamvla_amd.rollout import RolloutEngine
    monkeypatch.setattr(ops, "image_quality", _ref_image_quality)
    monkeypatch.setattr(ops, "depth_quality", _ref_depth_quality)
    B, T, h, n = 3, 11, 3, 11
    eng = RolloutEngine(_stub(obs_pred=True, depth_pred=True), B, use_graph=False, dreams=("image", "depth"), score_dreams=True, horizon=h)
    eng.device = torch.device("cpu")
    g = torch.Generator().manual_seed(11)
    dreams = torch.randint(0, 256, (T, B, 2, n, n, 3), generator=g, dtype=torch.uint8)
    frames = torch.randint(0, 256, (T, B, 2, n, n, 3), generator=g, dtype=torch.uint8)
    ddreams = torch.rand(T, B, 2, n, n, generator=g) + 0.5
    depths = torch.rand(T, B, 2, n, n, generator=g) + 0.5
    resets = {1: [False, False, True], 6: [False, True, False]}
    born = [0, 0, 0]                                                        # the step at which each episode last started
    for t in range(T):
        if t in resets:
            eng.reset(torch.tensor(resets[t]))
            born = [t if r else b0 for r, b0 in zip(resets[t], born)]
        eng.last_dreams = {"image": dreams[t], "depth": ddreams[t]}         # what the decode of this step left
        with_depth = t != 4
        eng._score(frames[t], depths[t] if with_depth else None)
        s = eng.last_dream_scores
        want_valid = [t - b0 >= h for b0 in born]
        assert s["valid"].tolist() == want_valid, (t, s["valid"])
        assert ("depth" in s) == with_depth and set(s) - {"depth"} == {"valid", "image", "persistence"}
        for b in range(B):
            for name, old in (("image", dreams), ("persistence", frames)):
                got = {k: v[b] for k, v in s[name].items()}
                assert all(tuple(v.shape) == (B, 2) for v in s[name].values())
                if want_valid[b]:
                    want = _ref_image_quality(old[t - h, b], frames[t, b])
                    assert all(torch.equal(got[k], want[k]) for k in ("sse", "mse", "psnr", "ssim")), (t, b, name)
                else:
                    assert got["sse"].tolist() == [-1, -1] and all(bool(torch.isnan(got[k]).all()) for k in ("mse", "psnr", "ssim"))
            if with_depth:
                got = {k: v[b] for k, v in s["depth"].items()}
                if want_valid[b]:
                    want = _ref_depth_quality(ddreams[t - h, b], depths[t, b])
                    assert all(torch.equal(got[k], want[k]) for k in want), (t, b)
                else:
                    assert got["valid"].tolist() == [-1, -1] and bool(torch.isnan(got["rmse"]).all())
    assert eng.since_reset.tolist() == [T - b0 for b0 in born]
    eng.reset()
    assert eng.since_reset.tolist() == [0, 0, 0]


def test_engine_rejects_frames_of_another_layout(monkeypatch):
    from dreamvla_amd.rollout import RolloutEngine
    eng = RolloutEngine(_stub(obs_pred=True), 2, use_graph=False, dreams=("image",), score_dreams=True)
    eng.device = torch.device("cpu")
    eng.last_dreams = {"image": torch.zeros(2, 2, 11, 11, 3, dtype=torch.uint8)}
    with pytest.raises(ValueError):
        eng._score(torch.zeros(2, 2, 3, 11, 11, dtype=torch.uint8), None)                    # CHW
    with pytest.raises(ValueError):
        eng._score(torch.zeros(2, 2, 11, 11, 3), None)                                       # not bytes
