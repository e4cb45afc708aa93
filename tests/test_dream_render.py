"""CPU: dreams at evaluation -- the torch restatement of the render (tests/dream_checks.py) pinned to the real reference's
`patchify` / `normalize_patchfied_image` / `unpatchify` through tests/golden/dream_render.pt (tests/make_golden_dream.py), the new
C-ABI entry points, and the `dreams` arguments of `DreamVLA.decode_tokens` and `RolloutEngine` (no GPU)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from tests import dream_checks as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return torch.load(os.path.join(ROOT, "tests", "golden", "dream_render.pt"), map_location="cpu")


def test_patch_helpers_match_the_reference(fx):
    P = fx["patch"]
    assert torch.equal(D.patchify(fx["imgs"], P), fx["patches"])
    assert torch.equal(D.normalize_patches(fx["patches"]), fx["normalized"])
    # the reference's unpatchify carries a pred_num axis: (B, P, patches, values) -> (B, P, C, H, W)
    assert torch.equal(D.unpatchify(fx["patches"], P, 3), fx["unpatchified"][:, 0])
    assert torch.equal(D.unpatchify(fx["depth_patches"][0], P, 1), fx["depth_unpatchified"][0])


def test_unpatchify_of_patchify_is_the_identity(fx):
    assert torch.equal(D.unpatchify(D.patchify(fx["imgs"], fx["patch"]), fx["patch"], 3), fx["imgs"])
    assert torch.equal(fx["unpatchified"][:, 0], fx["imgs"])


def test_render_without_current_is_the_reference_unpatchify(fx):
    P = fx["patch"]
    assert torch.equal(D.render_float(fx["normalized"], "image", P), fx["unpatchified_normalized"][:, 0])
    assert torch.equal(D.render_float(fx["depth_patches"][0], "depth", P), fx["depth_unpatchified"][0, :, 0])


def test_render_with_the_frame_itself_gives_the_frame_back(fx):
    """the head's target for a future frame equal to the current one, rendered against the current one: the frame again.  fp32:
    four roundings (x - mean, / sd, * sd, + mean), each at most 2^-24 of an operand no larger than 2 max|x|, and as much again for
    the two sides' statistics -- 16 x 2^-24 x max|x|.  The constant patch (variance 0: 1e-6 alone under the root) included."""
    img = fx["imgs"]
    back = D.render_frame(fx["normalized"], img, fx["patch"])
    err = float((back - img).abs().max())
    assert err <= 16 * 2.0 ** -24 * float(img.abs().max()), err
    # float64 on the fp32 data: the restatement as the GPU test evaluates it
    back64 = D.render_frame(D.normalize_patches(D.patchify(img.double(), fx["patch"])), img.double(), fx["patch"])
    assert float((back64 - img.double()).abs().max()) <= 1e-12
    # and down to the 0..255 levels the frames were made from
    from dreamvla_amd.preprocess import CLIP_MEAN, CLIP_STD
    u8 = D.render_u8(fx["normalized"], img, fx["patch"])
    want = torch.round((img * torch.tensor(CLIP_STD).view(3, 1, 1) + torch.tensor(CLIP_MEAN).view(3, 1, 1)) * 255).permute(0, 2, 3, 1)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (2, fx["side"], fx["side"], 3)
    assert torch.equal(u8.float(), want)


def test_levels_round_half_to_even():
    lv = torch.tensor([0.5, 1.5, 2.5, 254.5])
    assert torch.round(lv).tolist() == [0.0, 2.0, 2.0, 254.0]


def _header():
    txt = open(os.path.join(ROOT, "include", "dvla.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


C_TYPES = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const int64_t*": ctypes.c_void_p, "int64_t": ctypes.c_int64,
           "int32_t": ctypes.c_int32, "const float*": ctypes.POINTER(ctypes.c_float)}


@pytest.mark.parametrize("symbol", ["dvla_dream_render", "dvla_gather_positions"])
def test_new_entry_points_are_exported_and_bound_as_declared(symbol):
    from dreamvla_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, symbol)
    assert lib.dvla_abi_version() == 9                        # the version include/dvla.h declares
    decl = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % symbol, _header(), flags=re.S).group(1)
    want = []
    for arg in decl.split(","):
        typ = re.sub(r"\s*\b[A-Za-z_][A-Za-z0-9_]*\s*$", "", " ".join(arg.split()))       # drop the parameter name
        want.append(C_TYPES[typ.replace(" *", "*")])
    res, args = _lib.SYMBOLS[symbol]
    assert res is ctypes.c_int and list(args) == want


def test_dream_render_argument_rules():
    from dreamvla_amd import ops
    from dreamvla_amd._lib import DvlaError
    p = torch.zeros(1, 196, 768, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.dream_render(p, "picture")
    with pytest.raises(DvlaError):                            # no CPU fallback
        ops.dream_render(p, "image")
    feat = torch.zeros(1, 256, 256, dtype=torch.bfloat16)
    assert ops.dream_render(feat, "sam") is feat and ops.dream_render(feat, "dino") is feat and ops.dream_render(feat, "traj") is feat


def test_decode_tokens_takes_dreams_and_names_are_checked():
    from dreamvla_amd.dreamvla_model import DreamVLA
    sig = inspect.signature(DreamVLA.decode_tokens)
    assert sig.parameters["dreams"].default is None
    assert "dreams" not in inspect.signature(DreamVLA.forward).parameters          # forward is the reference's surface

    class Has:
        obs_pred, depth_pred, sam_feat_pred = True, True, True
        dino_feat_pred = trajectory_pred = False
    assert DreamVLA.dream_names(Has()) == ("image", "depth", "sam")
    assert DreamVLA._check_dreams(Has(), None) == () and DreamVLA._check_dreams(Has(), ()) == ()
    assert DreamVLA._check_dreams(Has(), ["sam", "image", "sam"]) == ("sam", "image")
    assert DreamVLA._check_dreams(Has(), "depth") == ("depth",)
    with pytest.raises(ValueError):
        DreamVLA._check_dreams(Has(), ("dino",))               # a head the model was not built with
    with pytest.raises(ValueError):
        DreamVLA._check_dreams(Has(), ("rgb",))                # not a dream at all


def test_engine_takes_dreams():
    from dreamvla_amd.rollout import RolloutEngine
    from tests.test_rollout_host_rules import _FakeDiTModel
    m = _FakeDiTModel()
    eng = RolloutEngine(m, 2, use_graph=False)
    assert eng.dreams == () and eng.last_dreams == {} and eng.frames is None
    with pytest.raises(ValueError):
        RolloutEngine(m, 2, use_graph=False, dreams=("image",))                     # the stand-in has no dream head
    m.obs_pred = m.sam_feat_pred = True
    eng = RolloutEngine(m, 2, use_graph=False, dreams=("image", "sam"))
    assert eng.dreams == ("image", "sam") and eng.dreams_all is False
    assert RolloutEngine(m, 2, use_graph=False, sample="all", dreams=["sam"]).dreams_all is True
    with pytest.raises(ValueError):
        RolloutEngine(m, 2, use_graph=False, dreams=("depth",))


def test_engine_keeps_the_frames_of_the_window():
    """the frame ring follows the token ring's rules (padding by the newest frame, sliding, reset): host logic, CPU tensors"""
    from dreamvla_amd.rollout import RolloutEngine
    from tests.rollout_checks import WindowOracle
    from tests.test_rollout_host_rules import _FakeDiTModel
    m = _FakeDiTModel()
    m.obs_pred = True
    B, S = 2, m.sequence_length
    for sample in ("newest", "all"):
        eng = RolloutEngine(m, B, use_graph=False, sample=sample, dreams=("image",))
        eng.device = torch.device("cpu")
        oracles = [WindowOracle(S) for _ in range(B)]
        for t in range(2 * S + 1):
            if t == S + 1:
                eng.reset(torch.tensor([True, False]))
                oracles[0] = WindowOracle(S)
            tok = torch.full((B, 3, 8), float(t))
            frames = torch.full((B, 2, 3, 4, 4), float(t)) + torch.arange(B).view(B, 1, 1, 1, 1) * 100
            eng._push(tok, frames)
            wins = [o.push(t)[0] for o in oracles]
            if sample == "newest":
                assert torch.equal(eng.frames, frames)
            else:
                for b in range(B):
                    assert eng.frames[b, :, 0, 0, 0, 0].tolist() == [float(f) + 100 * b for f in wins[b]]
                    assert eng.tokens[b, :, 0, 0].tolist() == [float(f) for f in wins[b]]
