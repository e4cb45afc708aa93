"""GPU: CLIP's bicubic Resize + CenterCrop on the device (csrc/image_resize.hip) against Pillow, byte for byte, and the two
callers that take raw camera frames: DeviceCollator(device_resize=True) and RolloutEngine.step_raw.

Bounds: the kernel does Pillow's integer arithmetic on Pillow's float64 tables, so every comparison here is equality -- the
expected number of differing bytes is 0 and nothing else passes.  Each row goes through tests.model_checks.report
($DVLA_PARITY_REPORT -> profiles/r10_parity_resize.jsonl).

Measured on an MI355X: 231 rows, 0 differing bytes / elements in every one of them (150 kernel rows over 10 sizes x 5 contents x
N = 1, 2, 128; 16 view / alignment / target-size rows; 16 collator rows; 49 engine rows, eager and hipGraph)."""
import numpy as np
import pytest
import torch

from dreamvla_amd import preprocess as P
from tests import model_checks as C
from tests.resize_cases import CONTENTS, SIZES, frames, pillow

POISON, GUARD = 0xA5, 4096


def _row(name, mismatches, ok=None, **kw):
    return dict(name=name, mismatches=int(mismatches), ok=bool(mismatches == 0 if ok is None else ok), **kw)


def _assert_all(results):
    C.report(results)
    bad = [r for r in results if not r["ok"]]
    assert not bad, bad


def _launch(src, out, n_px=224):
    """dvla_image_resize_u8 through the C ABI on caller-owned buffers (resize_frames_u8 allocates its own output)"""
    from dreamvla_amd import _lib
    from dreamvla_amd.ops import _stream
    n, h, w, _ = src.shape
    nh, nw, top, left = P._resize_geometry(h, w, n_px)
    bx, kx, ksx = P._tables_on(src.device, w, nw)
    by, ky, ksy = P._tables_on(src.device, h, nh)
    return _lib.load().dvla_image_resize_u8(src.data_ptr(), out.data_ptr(), n, h, w, nh, nw, bx.data_ptr(), kx.data_ptr(), ksx,
                                            by.data_ptr(), ky.data_ptr(), ksy, left, top, n_px, _stream())


def _guarded(n, n_px=224, shift=0):
    """an output of n frames inside a poisoned buffer: GUARD + shift bytes in front, GUARD - shift behind"""
    nbytes = n * n_px * n_px * 3
    buf = torch.full((nbytes + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD + shift:GUARD + shift + nbytes].view(n, n_px, n_px, 3)


def _guards_intact(buf, nbytes, shift=0):
    return bool((buf[:GUARD + shift] == POISON).all()) and bool((buf[GUARD + shift + nbytes:] == POISON).all())


@pytest.mark.gpu
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_pillow_byte_for_byte(hw):
    """every size x content at N = 1, 2 and 128 distinct frames (N = 1 / 2 are the first frames of the 128: a wrong frame stride or
    tile index shows at 2 and 128), into a poisoned output between sentinel regions, twice"""
    h, w = hw
    res = []
    for kind in CONTENTS:
        a = frames(h, w, kind, 128)
        want = torch.from_numpy(pillow(a))
        dev = torch.from_numpy(a).cuda()
        for n in (1, 2, 128):
            buf, out = _guarded(n)
            rc = _launch(dev[:n].contiguous(), out)
            torch.cuda.synchronize()
            first = out.cpu()
            bad = int((first != want[:n]).sum())
            # a value Pillow never produces here would hide unwritten bytes only if Pillow's own byte were the poison byte: count
            # the bytes still at the poison value against Pillow's count of that value
            unwritten = int((first == POISON).sum()) - int((want[:n] == POISON).sum())
            rc2 = _launch(dev[:n].contiguous(), out)
            torch.cuda.synchronize()
            again = int((out.cpu() != first).sum())
            ok = rc == 0 and rc2 == 0 and bad == 0 and unwritten == 0 and again == 0 and _guards_intact(buf, out.numel())
            res.append(_row(f"resize.kernel.{h}x{w}.{kind}.n{n} vs Pillow (differing bytes)", bad, ok, rc=rc, unwritten=unwritten,
                            second_run_differs=again, guards_intact=_guards_intact(buf, out.numel())))
    _assert_all(res)


@pytest.mark.gpu
def test_views_alignment_and_other_targets():
    res = []
    # a non-contiguous view: every second frame of a batch, and a window cut out of larger frames
    a = frames(200, 200, "noise", 6)
    got = P.resize_frames_u8(torch.from_numpy(a).cuda()[::2]).cpu()
    res.append(_row("resize.view.every_second_frame vs Pillow", int((got != torch.from_numpy(pillow(a[::2]))).sum())))
    big = frames(256, 256, "extreme", 3)
    view = torch.from_numpy(big).cuda()[:, 10:210, 31:231]
    assert not view.is_contiguous()
    got = P.resize_frames_u8(view).cpu()
    res.append(_row("resize.view.window_of_larger_frames vs Pillow", int((got != torch.from_numpy(pillow(big[:, 10:210, 31:231]))).sum())))
    # leading axes are kept: (B, T, h, w, 3) -> (B, T, 224, 224, 3)
    bt = frames(84, 84, "noise", 6).reshape(2, 3, 84, 84, 3)
    got = P.resize_frames_u8(torch.from_numpy(bt).cuda())
    assert tuple(got.shape) == (2, 3, 224, 224, 3)
    res.append(_row("resize.leading_axes vs Pillow", int((got.cpu().reshape(6, 224, 224, 3) != torch.from_numpy(pillow(bt.reshape(6, 84, 84, 3)))).sum())))
    # source and output at odd addresses (byte loads in front of the 16-byte body; the byte-store path of the output)
    for (h, w) in ((200, 200), (84, 84), (480, 640)):
        a = frames(h, w, "noise", 3)
        want = torch.from_numpy(pillow(a))
        for s_off, o_off in ((1, 0), (0, 1), (7, 13)):
            raw = torch.zeros(a.size + 16, dtype=torch.uint8, device="cuda")
            raw[s_off:s_off + a.size] = torch.from_numpy(a).cuda().flatten()
            src = raw[s_off:s_off + a.size].view(3, h, w, 3)
            buf, out = _guarded(3, shift=o_off)
            rc = _launch(src, out)
            torch.cuda.synchronize()
            bad = int((out.cpu() != want).sum())
            res.append(_row(f"resize.misaligned.{h}x{w}.src+{s_off}.out+{o_off} vs Pillow", bad,
                            rc == 0 and bad == 0 and _guards_intact(buf, out.numel(), o_off)))
    # another target size: rows of 3 * 225 = 675 bytes are not a multiple of 16 (byte stores, a partial last 16-byte chunk)
    a = frames(200, 200, "noise", 2)
    for n_px in (96, 225):
        want = torch.from_numpy(pillow(a, n_px))
        buf, out = _guarded(2, n_px)
        rc = _launch(torch.from_numpy(a).cuda(), out, n_px)
        torch.cuda.synchronize()
        bad = int((out.cpu() != want).sum())
        res.append(_row(f"resize.n_px{n_px} vs Pillow", bad, rc == 0 and bad == 0 and _guards_intact(buf, out.numel())))
        res.append(_row(f"resize.n_px{n_px} resize_frames_u8 vs Pillow", int((P.resize_frames_u8(torch.from_numpy(a).cuda(), n_px).cpu() != want).sum())))
    _assert_all(res)


@pytest.mark.gpu
def test_return_codes():
    from dreamvla_amd import _lib
    from dreamvla_amd.ops import _stream
    lib = _lib.load()
    src = torch.zeros(1, 200, 200, 3, dtype=torch.uint8, device="cuda")
    buf, out = _guarded(1)
    bx, kx, ks = P._tables_on(src.device, 200, 224)
    args = lambda **kw: [kw.get(k, v) for k, v in dict(src=src.data_ptr(), out=out.data_ptr(), n=1, h=200, w=200, nh=224, nw=224, bx=bx.data_ptr(),
                                                       kx=kx.data_ptr(), ksx=ks, by=bx.data_ptr(), ky=kx.data_ptr(), ksy=ks, left=0, top=0, n_px=224,
                                                       stream=_stream()).items()]
    assert lib.dvla_image_resize_u8(*args()) == 0
    assert lib.dvla_image_resize_u8(*args(n=0)) == 0
    for bad in (dict(src=None), dict(out=None), dict(bx=None), dict(ky=None), dict(n=-1), dict(h=0), dict(ksx=0), dict(left=1), dict(top=-1),
                dict(n_px=225)):
        assert lib.dvla_image_resize_u8(*args(**bad)) == -1, bad                      # DVLA_ERR_ARG
    # one output row's vertical taps alone exceed the LDS plan: a 40 000-row source (ksize 717 x 672 bytes)
    assert lib.dvla_image_resize_u8(*args(h=40000, ksy=717)) == -3                    # DVLA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert _guards_intact(buf, out.numel())


def _collators(rec, device_resize):
    from dreamvla_amd import collate
    from tests.collate_samples import fake_tokenize
    c = rec["case"]
    cls = collate.LiberoDeviceCollator if c["dataset"] == "libero" else collate.DeviceCollator
    col = cls(fake_tokenize, window_size=rec["window_size"], rgb_pad=c["rgb_pad"], gripper_pad=c["gripper_pad"], traj_cons=c["traj_cons"],
              act_step=c["act_step"], load_track_labels=c["load_track_labels"], device="cuda", device_resize=device_resize)
    col._shifts = lambda n, pad, key: rec["shifts"][key]           # the shifts the real collator drew (tests/test_collate.py)
    return col


@pytest.mark.gpu
def test_collator_device_resize_is_bit_equal():
    """entries 0 and 3 (static / gripper camera, 200 x 200 and 84 x 84 frames) of every case of tests/collate_samples.py -- pads 10 /
    4 / none, forward and forward_traj shifts, act_step cuts -- with the resize on the device against the resize in Pillow"""
    import os
    from tests.collate_samples import CASES, make_samples
    fx = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collate.pt"), weights_only=False)
    res = []
    for idx, case in enumerate(CASES):
        rec = fx["cases"][idx]
        assert rec["case"] == case
        host = _collators(rec, False)(make_samples(case))
        dev = _collators(rec, True)(make_samples(case))
        for e, name in ((0, "image"), (3, "gripper")):
            assert dev[e].is_cuda and dev[e].dtype == torch.bfloat16 and dev[e].shape == host[e].shape
            res.append(_row(f"resize.collator.{case['name']}.{name} device_resize vs host resize (differing elements)",
                            int((dev[e].view(torch.int16) != host[e].view(torch.int16)).sum()),
                            shifted=bool(case["rgb_pad" if e == 0 else "gripper_pad"] != -1)))
        for e in (1, 2, 4):
            assert torch.equal(dev[e], host[e])
    assert any(r["shifted"] for r in res) and not all(r["shifted"] for r in res)
    _assert_all(res)


def _engine_model(S):
    from dreamvla_amd.dreamvla_model import DreamVLA
    from oracle import weights
    cfg = dict(finetune_type="calvin", sequence_length=S, num_resampler_query=16, num_obs_token_per_image=9, action_pred_steps=3,
               transformer_layers=2, hidden_dim=1024, transformer_heads=16, phase="finetune", obs_pred=True, use_dit_head=True,
               attn_implementation="sdpa")
    m = DreamVLA(clip_device="cpu", vit_checkpoint_path=None, **cfg)
    m.load_state_dict(weights.fill_state_dict(m.state_dict()), strict=True)
    m = m.to(C.BF).to("cuda")
    m._init_model_type()
    return m.eval()


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_step_raw_equals_step_on_pillow_frames(use_graph):
    """S + 2 control steps of two engines on one model, one episode reset mid-way: `step_raw` on the raw 200 x 200 / 84 x 84 frames
    (host arrays, then device tensors) against `step` on the same frames resized by Pillow and normalised by preprocess_frames.
    The two engines see byte-equal inputs, so actions are compared with torch.equal; GEMM tuner trials are off so that both run
    the same kernels (a trial times a different configuration per call)."""
    from dreamvla_amd import ops
    from dreamvla_amd.rollout import RolloutEngine
    S, B = 4, 2
    m = _engine_model(S)
    res = []
    with ops.gemm_trials(False):
        raw_eng = RolloutEngine(m, B, use_graph=use_graph, warmup_decodes=2)
        ref_eng = RolloutEngine(m, B, use_graph=use_graph, warmup_decodes=2)
        g = torch.Generator().manual_seed(3)
        text = torch.randint(1, 49000, (B, 77), generator=g)
        text[:, 20] = 49407
        text[:, 21:] = 0
        for t in range(S + 2):
            if t == S - 1:
                mask = torch.tensor([False, True])
                raw_eng.reset(mask)
                ref_eng.reset(mask)
            prim, wrist = frames(200, 200, "noise", B, seed=t), frames(84, 84, "noise", B, seed=t)
            state = torch.cat([torch.rand(B, 6, generator=g), (torch.rand(B, 1, generator=g) > 0.5).float()], -1).to(C.BF)
            noise = torch.randn(B * S, 3, 7, generator=g).to(C.BF).float().cuda()
            if t % 2:                  # device tensors on odd steps, host arrays on even ones
                got = raw_eng.step_raw(torch.from_numpy(prim).cuda(), torch.from_numpy(wrist).cuda(), state, text, noise=noise)
            else:
                got = raw_eng.step_raw(prim, wrist, state, text, noise=noise)
            u8 = torch.from_numpy(np.stack((pillow(prim), pillow(wrist)), axis=1)).cuda()
            x = P.preprocess_frames(u8)
            want = ref_eng.step(x[:, 0], x[:, 1], state, text, noise=noise)
            tag = f"resize.step_raw.graph{int(use_graph)}.t{t}"
            res.append(_row(tag + ".last_frames_u8 vs Pillow (differing bytes)", int((raw_eng.last_frames_u8 != u8).sum())))
            for nm, a_, b_ in zip(("action", "arm", "gripper"), got, want):
                same = a_.shape == b_.shape and a_.dtype == b_.dtype and torch.equal(a_, b_)
                res.append(_row(f"{tag}.{nm} step_raw vs step (differing elements)", int((a_ != b_).sum()) if a_.shape == b_.shape else -1,
                                same and bool(torch.isfinite(a_.float()).all())))
        if use_graph:
            res.append(_row("resize.step_raw.graphs_captured", 0, raw_eng.graphs_captured and ref_eng.graphs_captured))
    assert tuple(raw_eng.last_frames_u8.shape) == (B, 2, 224, 224, 3) and raw_eng.last_frames_u8.dtype == torch.uint8
    _assert_all(res)
