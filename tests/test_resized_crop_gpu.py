"""GPU: the per-frame resized crop + flip (csrc/image_resized_crop.hip) against Pillow, byte for byte, its fused bf16 kind against
preprocess_frames of the uint8 kind, bit for bit, and MAEFrameAugment in front of a small MaskedAutoencoderViT.

Bounds: the kernel does Pillow's integer arithmetic on Pillow's float64 tables and torch's fp32 operation order behind it, so every
comparison here is equality -- the expected number of differing bytes / elements is 0 and nothing else passes.  Each row goes
through tests.model_checks.report ($DVLA_PARITY_REPORT -> profiles/r13_parity_resized_crop.jsonl).

Shapes: 32 frames per launch (8 edge crops + 24 drawn ones: tests/resized_crop_cases.py) of the four source sizes, the smallest at
which the frame stride, the table directory, mixed tap counts (5 taps up-scaling next to 11 / 13 down-scaling a whole 480 x 640
frame), the identity pass, a segment at every alignment and the flip meet in one launch.

Measured on an MI355X: 81 rows, 0 differing bytes / elements in every one of them; the file runs in about 4 s."""
import ctypes

import pytest
import torch

from dreamvla_amd import preprocess as P
from tests import model_checks as C
from tests.resize_cases import frames
from tests.resized_crop_cases import SOURCES, crops_for, edge_crops, pillow_crops

POISON, GUARD = 0xA5, 4096
OTHER_MEAN, OTHER_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # ImageNet's, the MAE recipe's own


def _row(name, mismatches, ok=None, **kw):
    return dict(name=name, mismatches=int(mismatches), ok=bool(mismatches == 0 if ok is None else ok), **kw)


def _assert_all(results):
    C.report(results)
    bad = [r for r in results if not r["ok"]]
    assert not bad, bad


def _launch(src, crops, out, n_px=224, mean=None, std=None):
    """dvla_image_resized_crop through the C ABI on a caller-owned output (resized_crop_u8 / resized_crop allocate their own); the
    boxes pass the host check of the public functions first: no launch ever sees a box outside its frame"""
    from dreamvla_amd import _lib
    from dreamvla_amd.ops import _stream
    n, h, w, _ = src.shape
    boxes, max_ch, max_cw = P._check_crops(crops, n, h, w, "test")
    store, max_size = P._crop_table_store(src.device, h, w, n_px)
    dev = boxes.to(src.device)
    bf = out.dtype == torch.bfloat16
    m3 = (ctypes.c_float * 3)(*mean) if bf else None
    s3 = (ctypes.c_float * 3)(*std) if bf else None
    return _lib.load().dvla_image_resized_crop(src.data_ptr(), out.data_ptr(), dev.data_ptr(), store.data_ptr(), n, h, w, max_size, max_ch,
                                               max_cw, n_px, _lib.CROP_OUT_BF16 if bf else _lib.CROP_OUT_U8, m3, s3, _stream())


def _guarded(n, n_px=224, shift=0, bf16=False):
    """an output of n frames inside a poisoned byte buffer: GUARD + shift bytes in front, GUARD - shift behind"""
    nbytes = n * n_px * n_px * 3 * (2 if bf16 else 1)
    buf = torch.full((nbytes + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
    body = buf[GUARD + shift:GUARD + shift + nbytes]
    return buf, (body.view(torch.bfloat16).view(n, 3, n_px, n_px) if bf16 else body.view(n, n_px, n_px, 3))


def _guards_intact(buf, nbytes, shift=0):
    return bool((buf[:GUARD + shift] == POISON).all()) and bool((buf[GUARD + shift + nbytes:] == POISON).all())


_cases = {}


def _case(h, w, kind):
    """32 frames, their 32 crops and Pillow's result: computed once, shared, never written"""
    key = (h, w, kind)
    if key not in _cases:
        a, crops = frames(h, w, kind, 32), crops_for(h, w, 24)
        _cases[key] = (a, crops, torch.from_numpy(pillow_crops(a, crops)), torch.from_numpy(a).cuda())
    return _cases[key]


@pytest.mark.gpu
@pytest.mark.parametrize("hw", SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_pillow_byte_for_byte(hw):
    """every content at n = 1, 2 and 32 distinct frames with distinct boxes (n = 1 / 2 are the first frames of the 32: a wrong frame
    or descriptor stride shows at 2 and 32), into a poisoned output between sentinel regions, twice"""
    h, w = hw
    res = []
    for kind in ("noise", "extreme", "ramps"):
        a, crops, want, dev = _case(h, w, kind)
        assert set(crops[:, 4].tolist()) == {0, 1}
        if hw in ((300, 225), (480, 640)):     # down-scaling, up-scaling and the identity pass in one launch
            assert bool((crops[:, 2] > 224).any()) and bool((crops[:, 2] < 224).any()) and bool((crops[:, 2:4] == 224).any())
        for n in (1, 2, 32):
            buf, out = _guarded(n)
            rc = _launch(dev[:n], crops[:n], out)
            torch.cuda.synchronize()
            first = out.cpu()
            bad = int((first != want[:n]).sum())
            # unwritten bytes hide behind Pillow's own 0xA5 bytes only: count the poison value against Pillow's count of it
            unwritten = int((first == POISON).sum()) - int((want[:n] == POISON).sum())
            rc2 = _launch(dev[:n], crops[:n], out)
            torch.cuda.synchronize()
            again = int((out.cpu() != first).sum())
            intact = _guards_intact(buf, out.numel())
            ok = rc == 0 and rc2 == 0 and bad == 0 and unwritten == 0 and again == 0 and intact
            res.append(_row(f"resized_crop.kernel.{h}x{w}.{kind}.n{n} vs Pillow (differing bytes)", bad, ok, rc=rc, unwritten=unwritten,
                            second_run_differs=again, guards_intact=intact))
    _assert_all(res)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fused_bf16_kind_equals_preprocess_frames_bit_for_bit(hw):
    h, w = hw
    a, crops, want, dev = _case(h, w, "noise")
    res = []
    for tag, mean, std in (("clip", P.CLIP_MEAN, P.CLIP_STD), ("imagenet", OTHER_MEAN, OTHER_STD)):
        ref = P.preprocess_frames(P.resized_crop_u8(dev, crops), mean=mean, std=std)
        ref_pillow = P.preprocess_frames(want.cuda(), mean=mean, std=std)
        buf, out = _guarded(32, bf16=True)
        rc = _launch(dev, crops, out, mean=mean, std=std)
        torch.cuda.synchronize()
        bad = int((out.view(torch.int16) != ref.view(torch.int16)).sum())
        bad_pillow = int((out.view(torch.int16) != ref_pillow.view(torch.int16)).sum())
        intact = _guards_intact(buf, out.numel() * 2)
        res.append(_row(f"resized_crop.bf16.{h}x{w}.{tag} vs preprocess_frames(resized_crop_u8) (differing elements)", bad,
                        rc == 0 and bad == 0 and bad_pillow == 0 and intact, rc=rc, vs_pillow_then_preprocess=bad_pillow, guards_intact=intact))
        got = P.resized_crop(dev, crops, mean=mean, std=std)
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == (32, 3, 224, 224)
        res.append(_row(f"resized_crop.bf16.{h}x{w}.{tag} resized_crop() vs the guarded launch", int((got.view(torch.int16) != out.view(torch.int16)).sum())))
    _assert_all(res)


@pytest.mark.gpu
def test_flip_reverses_the_output_columns():
    res = []
    for (h, w) in ((200, 200), (300, 225)):
        a, crops, _, dev = _case(h, w, "noise")
        c0, c1 = crops.clone(), crops.clone()
        c0[:, 4], c1[:, 4] = 0, 1
        u0, u1 = P.resized_crop_u8(dev, c0), P.resized_crop_u8(dev, c1)
        res.append(_row(f"resized_crop.flip.{h}x{w}.u8 flip=1 vs flip=0 reversed", int((u1 != u0.flip(-2)).sum())))
        b0, b1 = P.resized_crop(dev, c0), P.resized_crop(dev, c1)
        res.append(_row(f"resized_crop.flip.{h}x{w}.bf16 flip=1 vs flip=0 reversed", int((b1.view(torch.int16) != b0.flip(-1).view(torch.int16)).sum())))
        assert int((u0 != u0.flip(-2)).sum()) > 0               # the frames are not mirror-symmetric: the comparison can fail
    _assert_all(res)


@pytest.mark.gpu
def test_a_frame_does_not_depend_on_its_batch():
    res = []
    for (h, w) in ((84, 84), (480, 640)):
        a, crops, _, dev = _case(h, w, "noise")
        batch_u8, batch_bf = P.resized_crop_u8(dev, crops), P.resized_crop(dev, crops)
        bad_u8 = bad_bf = 0
        for i in range(32):      # alone, the launch's LDS plan is made for this frame's crop, not for the batch's largest
            bad_u8 += int((P.resized_crop_u8(dev[i:i + 1], crops[i:i + 1]) != batch_u8[i:i + 1]).sum())
            bad_bf += int((P.resized_crop(dev[i:i + 1], crops[i:i + 1]).view(torch.int16) != batch_bf[i:i + 1].view(torch.int16)).sum())
        res.append(_row(f"resized_crop.independence.{h}x{w}.u8 alone vs in the batch of 32", bad_u8))
        res.append(_row(f"resized_crop.independence.{h}x{w}.bf16 alone vs in the batch of 32", bad_bf))
    _assert_all(res)


@pytest.mark.gpu
def test_views_alignment_and_other_targets():
    res = []
    # a non-contiguous view: every second frame of a batch, and a window cut out of larger frames
    a, crops = frames(200, 200, "noise", 6), crops_for(200, 200, 0)[[0, 3, 7]]
    got = P.resized_crop_u8(torch.from_numpy(a).cuda()[::2], crops).cpu()
    res.append(_row("resized_crop.view.every_second_frame vs Pillow", int((got != torch.from_numpy(pillow_crops(a[::2], crops))).sum())))
    big = frames(256, 256, "extreme", 3)
    view = torch.from_numpy(big).cuda()[:, 10:210, 31:231]
    assert not view.is_contiguous()
    want = torch.from_numpy(pillow_crops(big[:, 10:210, 31:231], crops))
    res.append(_row("resized_crop.view.window_of_larger_frames vs Pillow", int((P.resized_crop_u8(view, crops).cpu() != want).sum())))
    res.append(_row("resized_crop.view.window_of_larger_frames bf16 vs preprocess_frames(Pillow)",
                    int((P.resized_crop(view, crops).view(torch.int16) != P.preprocess_frames(want.cuda()).view(torch.int16)).sum())))
    # leading axes are kept: (B, T, h, w, 3) -> (B, T, 224, 224, 3) and (B, T, 3, 224, 224)
    bt, crops6 = frames(84, 84, "noise", 6), crops_for(84, 84, 0)[2:8]
    want = torch.from_numpy(pillow_crops(bt, crops6))
    dev = torch.from_numpy(bt.reshape(2, 3, 84, 84, 3)).cuda()
    got, got_bf = P.resized_crop_u8(dev, crops6), P.resized_crop(dev, crops6)
    assert tuple(got.shape) == (2, 3, 224, 224, 3) and tuple(got_bf.shape) == (2, 3, 3, 224, 224)
    res.append(_row("resized_crop.leading_axes vs Pillow", int((got.cpu().reshape(6, 224, 224, 3) != want).sum())))
    res.append(_row("resized_crop.leading_axes bf16 vs preprocess_frames(Pillow)",
                    int((got_bf.reshape(6, 3, 224, 224).view(torch.int16) != P.preprocess_frames(want.cuda()).view(torch.int16)).sum())))
    # source and output at odd addresses (byte loads in front of the 16-byte body; the byte-store path of the output)
    for (h, w) in ((200, 200), (84, 84), (480, 640)):
        a, crops8 = frames(h, w, "noise", 8), crops_for(h, w, 0)
        want = torch.from_numpy(pillow_crops(a, crops8))
        for s_off, o_off in ((1, 0), (0, 1), (7, 13)):
            raw = torch.zeros(a.size + 16, dtype=torch.uint8, device="cuda")
            raw[s_off:s_off + a.size] = torch.from_numpy(a).cuda().flatten()
            src = raw[s_off:s_off + a.size].view(8, h, w, 3)
            buf, out = _guarded(8, shift=o_off)
            rc = _launch(src, crops8, out)
            torch.cuda.synchronize()
            bad = int((out.cpu() != want).sum())
            res.append(_row(f"resized_crop.misaligned.{h}x{w}.src+{s_off}.out+{o_off} vs Pillow", bad,
                            rc == 0 and bad == 0 and _guards_intact(buf, out.numel(), o_off)))
    # other target sizes: rows of 3 * 225 = 675 bytes are not a multiple of 16 (byte stores, a partial last 16-byte chunk)
    a = frames(200, 200, "noise", 8)
    for n_px in (96, 225):
        crops8 = torch.tensor(edge_crops(200, 200, n_px), dtype=torch.int32)
        want = torch.from_numpy(pillow_crops(a, crops8, n_px))
        buf, out = _guarded(8, n_px)
        rc = _launch(torch.from_numpy(a).cuda(), crops8, out, n_px)
        torch.cuda.synchronize()
        bad = int((out.cpu() != want).sum())
        res.append(_row(f"resized_crop.n_px{n_px} vs Pillow", bad, rc == 0 and bad == 0 and _guards_intact(buf, out.numel())))
        res.append(_row(f"resized_crop.n_px{n_px} resized_crop_u8 vs Pillow", int((P.resized_crop_u8(torch.from_numpy(a).cuda(), crops8, n_px).cpu() != want).sum())))
    got = P.resized_crop(torch.from_numpy(a).cuda(), torch.tensor(edge_crops(200, 200, 96), dtype=torch.int32), 96)
    want = P.preprocess_frames(torch.from_numpy(pillow_crops(a, edge_crops(200, 200, 96), 96)).cuda())
    res.append(_row("resized_crop.n_px96 bf16 vs preprocess_frames(Pillow)", int((got.view(torch.int16) != want.view(torch.int16)).sum())))
    _assert_all(res)


@pytest.mark.gpu
def test_arguments_are_refused_before_any_launch():
    from dreamvla_amd import _lib
    from dreamvla_amd.ops import _stream
    lib = _lib.load()
    src = torch.zeros(2, 200, 200, 3, dtype=torch.uint8, device="cuda")
    good = torch.tensor([[0, 0, 200, 200, 0], [3, 4, 5, 6, 1]], dtype=torch.int32)
    for fn in (P.resized_crop_u8, P.resized_crop):
        for bad in ([[0, 0, 201, 200, 0], [0, 0, 1, 1, 0]], [[0, 1, 200, 200, 0], [0, 0, 1, 1, 0]], [[0, 0, 0, 5, 0], [0, 0, 1, 1, 0]],
                    [[0, 0, 5, 5, 2], [0, 0, 1, 1, 0]], [[0, 0, 5, 5, 0]]):
            with pytest.raises(ValueError):
                fn(src, torch.tensor(bad, dtype=torch.int32))
        with pytest.raises(TypeError):
            fn(src, good.cuda())                               # the descriptors are a host tensor
        assert fn(src[:0], good[:0]).shape[0] == 0
    # the C entry point's own argument checks (valid descriptors throughout)
    buf, out = _guarded(2)
    store, max_size = P._crop_table_store(src.device, 200, 200, 224)
    dev = good.cuda()
    m3 = (ctypes.c_float * 3)(*P.CLIP_MEAN)
    args = lambda **kw: [kw.get(k, v) for k, v in dict(src=src.data_ptr(), out=out.data_ptr(), crops=dev.data_ptr(), store=store.data_ptr(), n=2,
                                                       h=200, w=200, max_size=max_size, max_ch=200, max_cw=200, n_px=224, kind=_lib.CROP_OUT_U8,
                                                       mean=None, std=None, stream=_stream()).items()]
    assert lib.dvla_image_resized_crop(*args()) == 0
    assert lib.dvla_image_resized_crop(*args(n=0)) == 0
    for bad in (dict(src=None), dict(out=None), dict(crops=None), dict(store=None), dict(n=-1), dict(h=0), dict(n_px=0), dict(max_ch=0),
                dict(max_ch=201), dict(max_cw=201), dict(max_size=199), dict(kind=2), dict(kind=_lib.CROP_OUT_BF16)):
        assert lib.dvla_image_resized_crop(*args(**bad)) == -1, bad                       # DVLA_ERR_ARG
    assert lib.dvla_image_resized_crop(*args(kind=_lib.CROP_OUT_BF16, mean=m3, std=m3, n_px=225)) == -3      # DVLA_ERR_UNSUPPORTED
    assert lib.dvla_image_resized_crop(*args(kind=_lib.CROP_OUT_BF16, mean=m3, std=m3, out=out.data_ptr() + 2)) == -3
    assert lib.dvla_image_resized_crop(*args(store=store.data_ptr() + 4)) == -3
    torch.cuda.synchronize()
    assert _guards_intact(buf, out.numel())


@pytest.mark.gpu
def test_mae_frame_augment_feeds_the_autoencoder():
    from dreamvla_amd.nn import LayerNorm
    from dreamvla_amd.vit_mae import MAEFrameAugment, MaskedAutoencoderViT
    torch.manual_seed(0)
    a = frames(84, 84, "noise", 8)
    dev = torch.from_numpy(a).cuda()
    aug = MAEFrameAugment(generator=torch.Generator().manual_seed(11))
    imgs = aug(dev)
    crops = aug.last_crops
    assert imgs.dtype == torch.bfloat16 and tuple(imgs.shape) == (8, 3, 224, 224) and tuple(crops.shape) == (8, 5)
    assert torch.equal(crops, P.draw_resized_crops(8, 84, 84, generator=torch.Generator().manual_seed(11)))
    want = P.preprocess_frames(torch.from_numpy(pillow_crops(a, crops)).cuda())
    res = [_row("resized_crop.mae_augment.imgs vs preprocess_frames(Pillow) (differing elements)", int((imgs.view(torch.int16) != want.view(torch.int16)).sum()))]
    assert not torch.equal(aug(dev), imgs) or not torch.equal(aug.last_crops, crops)      # the next call draws new boxes
    mae = MaskedAutoencoderViT(img_size=224, patch_size=16, embed_dim=128, depth=2, num_heads=2, decoder_embed_dim=64, decoder_depth=1,
                               decoder_num_heads=2, norm_layer=lambda d: LayerNorm(d, eps=1e-6)).to(torch.bfloat16).cuda()
    loss, pred, mask = mae(imgs, mask_ratio=0.75)
    loss.backward()
    grads = [p.grad for p in mae.parameters() if p.requires_grad and p.grad is not None]
    finite = bool(torch.isfinite(loss.float()).all()) and len(grads) > 0 and all(bool(torch.isfinite(g.float()).all()) for g in grads)
    res.append(_row("resized_crop.mae_augment.loss and gradients finite", 0, finite, loss=float(loss.detach())))
    assert tuple(pred.shape) == (8, 196, 768) and tuple(mask.shape) == (8, 196)
    _assert_all(res)
