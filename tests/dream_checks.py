"""Dreams at evaluation: the torch restatement of the render (pinned to the real reference's patch helpers by
tests/test_dream_render.py through tests/golden/dream_render.pt) and the GPU checks of tests/test_dream_rollout_gpu.py --
`decode_tokens(mode="test", dreams=...)` against the real reference's train-mode outputs, the selection of the executed position,
the render kernel against the restatement in float64, and the rollout engine's `last_dreams`."""
import torch

from dreamvla_amd.preprocess import CLIP_MEAN, CLIP_STD

SLOT = {"image": 2, "depth": 6, "traj": 7, "dino": 8, "sam": 9}       # positions in the model's 10-tuple


# ---------------------------------------------------------------------------------------------------
# restatement (any float dtype; CPU or GPU)
# ---------------------------------------------------------------------------------------------------
def patchify(imgs, patch):
    """(n, C, H, W) -> (n, gh * gw, patch * patch * C), the values of a patch in (p, q, c) order"""
    n, C, H, W = imgs.shape
    gh, gw = H // patch, W // patch
    x = imgs.reshape(n, C, gh, patch, gw, patch).permute(0, 2, 4, 3, 5, 1)
    return x.reshape(n, gh * gw, patch * patch * C)


def unpatchify(patches, patch, channels):
    """(n, gh * gw, patch * patch * C) -> (n, C, H, W); square grid"""
    n, L, D = patches.shape
    g = int(round(L ** 0.5))
    assert g * g == L and D == patch * patch * channels
    x = patches.reshape(n, g, g, patch, patch, channels).permute(0, 5, 1, 3, 2, 4)
    return x.reshape(n, channels, g * patch, g * patch)


def normalize_patches(p):
    mean = p.mean(dim=-1, keepdim=True)
    var = p.var(dim=-1, keepdim=True)                     # unbiased
    return (p - mean) / (var + 1.e-6) ** .5


def render_float(pred, kind, patch=16):
    """ops.dream_render without `current`: image -> (n, 3, H, W), depth -> (n, H, W)"""
    if kind == "image":
        return unpatchify(pred, patch, 3)
    return unpatchify(pred, patch, 1)[:, 0]


def render_frame(pred, current, patch=16):
    """the image prediction in the model's input space: the per-patch normalisation inverted with the statistics of the same
    patch of `current` (n, 3, H, W) -> (n, 3, H, W)"""
    cp = patchify(current, patch)
    mean = cp.mean(dim=-1, keepdim=True)
    var = cp.var(dim=-1, keepdim=True)
    return unpatchify(pred * (var + 1.e-6) ** .5 + mean, patch, 3)


def render_levels(pred, current, patch=16):
    """0..255 before rounding, HWC (n, H, W, 3)"""
    x = render_frame(pred, current, patch)
    mean = torch.tensor(CLIP_MEAN, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    return ((x * std + mean).clamp(0, 1) * 255).permute(0, 2, 3, 1)


def render_u8(pred, current, patch=16):
    return torch.round(render_levels(pred, current, patch)).to(torch.uint8)          # torch.round: half to even


# ---------------------------------------------------------------------------------------------------
# GPU checks
# ---------------------------------------------------------------------------------------------------
PAIR = 2.0           # two bf16 computations of one function, each within the fixture's bound of the reference (tests/rollout_checks.py)
TIE_MARGIN = 0.012   # levels: a 768-term fp32 sum has relative error <= 768 x 2^-24 = 4.6e-5, times 255 levels
FLOAT_BOUND = 768 * 2.0 ** -24     # x the magnitude of the output: fp32 round-off of the 768-term reduction length


def _row(name, value, tol, ok=None, **kw):
    return dict({"name": name, "rel_l2": float(value), "tol": float(tol), "ok": bool(value <= tol if ok is None else ok)}, **kw)


def _model(name):
    from tests.model_checks import BF, build_hip_model, golden_inputs, load
    fx = load(f"dreamvla_{name}.pt")
    m = build_hip_model(fx["cfg"]).to(BF).to("cuda")
    m._init_model_type()
    m.eval()
    inp = {k: v.to("cuda") for k, v in golden_inputs(fx).items()}
    return fx, m, (inp["image_primary"].to(BF), inp["image_wrist"].to(BF), inp["state"].to(BF), inp["text_token"])


def _dream_tuple(out):
    return tuple(o if i in SLOT.values() else None for i, o in enumerate(out))


def _pair(name, got, want, t_rel, t_abs):
    d = got.float() - want.float()
    r = float(d.norm() / max(float(want.float().norm()), 1e-12))
    worst = float(d.abs().max())
    return {"name": name, "rel_l2": r, "tol": PAIR * t_rel, "max_abs": worst, "max_abs_tol": PAIR * t_abs,
            "ok": bool(r <= PAIR * t_rel and worst <= PAIR * t_abs)}


def gpu_dream_head_checks(name, positions=None):
    """decode_tokens(mode="test", dreams=every head the model has) against fx["train"] -- the real reference's train-mode outputs
    of an eval() model under no_grad: the same trunk, the same heads -- at the bounds the train-mode checks apply
    (model_checks.compare_outputs with the fixture's records); the actions bit for bit those of a call without dreams; and the
    selected position (test_select) against the rows of the all-position call and against the fixture's samples in its slice."""
    from dreamvla_amd import ops
    from tests.model_checks import TOL_MODEL, compare_outputs, output_tolerances, rel_l2
    fx, m, args = _model(name)
    S, B = fx["S"], fx["B"]
    names = m.dream_names()
    dit = bool(fx["cfg"]["use_dit_head"])
    tn = fx["test_noise"].to("cuda") if dit else None
    res = []
    with torch.no_grad(), ops.gemm_trials(False):         # both calls on the same GEMM configurations: no tuner trials in between
        parts = m.encode_frames(*args)
        base = m.decode_tokens(parts, mode="test", test_noise=tn)
        out = m.decode_tokens(parts, mode="test", test_noise=tn, dreams=names)
        res.append(_row(f"dream.{name}.without dreams every dream slot is None", 0, 0, ok=all(base[i] is None for i in SLOT.values())))
        for i, nm in ((0, "arm"), (1, "gripper")):
            res.append(_row(f"dream.{name}.{nm} action bit-identical with and without dreams", 0, 0, ok=torch.equal(out[i], base[i])))
        want = [w if i in SLOT.values() else None for i, w in enumerate(fx["train"])]
        covered = [k for k in names if want[SLOT[k]] is not None]
        res.append(_row(f"dream.{name}.fixture covers {covered}", 0, 0, ok=sorted(covered) == sorted(names)))
        res += compare_outputs(_dream_tuple(out), want, TOL_MODEL, f"dream.{name}.all_positions_vs_real_reference", fx=fx)
        tols = output_tolerances(fx, TOL_MODEL)
        for pos in (positions if positions is not None else sorted({0, S // 2, S - 1})):
            sel = torch.full((B,), pos, dtype=torch.long, device="cuda")
            one = m.decode_tokens(parts, mode="test", test_noise=None if tn is None else tn.view(B, S, *tn.shape[1:])[:, pos],
                                  test_select=sel, dreams=names)
            for k in names:
                i = SLOT[k]
                t_rel, t_abs, _ = tols[i]
                full = out[i].view(B, S, *out[i].shape[1:])[:, pos]
                ok_shape = tuple(one[i].shape) == tuple(full.shape)
                res.append(_row(f"dream.{name}.select{pos}.{k} shape {tuple(one[i].shape)}", 0, 0, ok=ok_shape))
                res.append(_pair(f"dream.{name}.select{pos}.{k} vs the all-position call", one[i], full, t_rel, t_abs))
                rec = fx["train"][i]
                per = one[i][0].numel()                   # B = 1: position `pos` owns flat indices [pos * per, (pos + 1) * per)
                assert B == 1 and rec["shape"][0] == S
                inside = (rec["idx"] >= pos * per) & (rec["idx"] < (pos + 1) * per)
                n_in = int(inside.sum())
                gv = one[i].float().cpu().flatten()[rec["idx"][inside] - pos * per]
                wv = rec["vals"][inside]
                r = rel_l2(gv, wv) if n_in else float("inf")
                worst = float((gv - wv).abs().max()) if n_in else float("inf")
                res.append({"name": f"dream.{name}.select{pos}.{k} vs the real reference's {n_in} samples of that position",
                            "rel_l2": r, "tol": t_rel, "max_abs": worst, "max_abs_tol": t_abs,
                            "ok": bool(n_in > 0 and r <= t_rel and worst <= t_abs)})
    return res


def _render_case(tag, pred_img, cur, pred_depth, stats):
    """the three render modes on one set of bf16 inputs against the restatement in float64"""
    from dreamvla_amd import ops
    res = []
    p64, c64 = pred_img.double(), cur.double()
    got = ops.dream_render(pred_img, "image", cur)
    again = ops.dream_render(pred_img, "image", cur)
    res.append(_row(f"{tag}.u8 same launch twice bit-identical", 0, 0, ok=torch.equal(got, again)))
    res.append(_row(f"{tag}.u8 shape / dtype", 0, 0, ok=got.dtype == torch.uint8 and tuple(got.shape) == (cur.shape[0], cur.shape[2], cur.shape[3], 3)))
    lv = render_levels(p64, c64)
    want = torch.round(lv)
    diff = (got.double() - want).abs()
    differs = diff > 0
    tie_dist = ((lv - torch.floor(lv)) - 0.5).abs()
    worst_tie = float(tie_dist[differs].max()) if bool(differs.any()) else 0.0
    share = float(differs.double().mean())
    print(f"[dream render] {tag}: {int(differs.sum())} of {differs.numel()} pixels differ from the float64 rounding (share {share:.3g}); "
          f"max level difference {float(diff.max())}; furthest from a tie among them {worst_tie:.3g}", flush=True)
    res.append(_row(f"{tag}.u8 no pixel more than one level off", float(diff.max()), 1.0))
    res.append(_row(f"{tag}.u8 every differing pixel within {TIE_MARGIN} level of a rounding tie (share of pixels {share:.3g})", worst_tie, TIE_MARGIN))
    stats[f"{tag}.u8_share_differing"] = share
    stats[f"{tag}.u8_max_tie_distance"] = worst_tie
    for kind, pred in (("image", pred_img), ("depth", pred_depth)):
        g1 = ops.dream_render(pred, kind)
        g2 = ops.dream_render(pred, kind)
        w = render_float(pred.double(), kind)
        err = float((g1.double() - w).abs().max())
        bound = FLOAT_BOUND * max(float(w.abs().max()), 1.0)
        stats[f"{tag}.{kind}_float_max_err"] = err
        print(f"[dream render] {tag}: {kind} float32 output: max |error| {err:.3g} (bound {bound:.3g})", flush=True)
        res.append(_row(f"{tag}.{kind} float32 vs float64 restatement (max abs)", err, bound,
                        ok=err <= bound and g1.dtype == torch.float32 and tuple(g1.shape) == tuple(w.shape)))
        res.append(_row(f"{tag}.{kind} float32 same launch twice bit-identical", 0, 0, ok=torch.equal(g1, g2)))
    return res


def gpu_dream_render_checks(name="C", stats=None):
    """the render kernel on a fixture's frames and its model's predictions, and on one random case (predictions beyond the head's
    usual range, so that the clamp at both ends is exercised; a constant patch in the current frame)"""
    from dreamvla_amd import _lib, ops
    stats = {} if stats is None else stats
    fx, m, args = _model(name)
    with torch.no_grad():
        out = m.decode_tokens(m.encode_frames(*args), mode="test", test_noise=fx["test_noise"].to("cuda"), dreams=("image", "depth"))
    img = out[2][:, :, 0]                                   # (S, 2, 196, 768)
    cur = torch.stack((args[0][0], args[1][0]), dim=1)      # (S, 2, 3, 224, 224)
    res = _render_case(f"dream.render.{name}", img.reshape(-1, 196, 768), cur.reshape(-1, 3, 224, 224),
                       out[6][:, :, 0].reshape(-1, 196, 256), stats)
    g = torch.Generator().manual_seed(31)
    n = 5
    pred = (torch.randn(n, 196, 768, generator=g) * 1.5).to(torch.bfloat16).to("cuda")
    cur = (torch.randn(n, 3, 224, 224, generator=g) * 0.8 + 0.2).to(torch.bfloat16)
    cur[0, :, :16, :16] = 1.0
    depth = (torch.rand(n, 196, 256, generator=g) * 4).to(torch.bfloat16).to("cuda")
    res += _render_case("dream.render.random", pred, cur.to("cuda"), depth, stats)
    # what the kernel does not cover is refused, not computed wrongly
    refused = False
    try:
        ops.dream_render(pred[:, :, :8 * 8 * 3].contiguous(), "image", patch=8)
    except _lib.DvlaError:
        refused = True
    res.append(_row("dream.render.patch 8 is refused (DVLA_ERR_UNSUPPORTED)", 0, 0, ok=refused))
    return res


def _level_bound(frames, t_abs):
    """element-wise bound, in levels, between two renders whose bf16 predictions differ by at most PAIR x t_abs: the render is
    affine in the prediction with slope 255 x std_c x sqrt(var_patch + 1e-6) <= 255 x max std_c x the largest patch deviation of
    these frames; rounding adds at most one level"""
    sd = float((patchify(frames.reshape(-1, *frames.shape[-3:]).float(), 16).var(dim=-1) + 1e-6).sqrt().max())
    return 1.0 + 255.0 * max(CLIP_STD) * sd * PAIR * t_abs


def gpu_dream_engine_checks(name, use_graph, sample, episodes=1, slot=0, reset_at=None, extra_steps=0):
    """RolloutEngine(dreams=every head): frames of fixture `name` pushed one control step at a time into episode `slot` of
    `episodes` (the others get random frames).  Every step: `last_dreams` against the module-level call on the same (padded) window
    -- decode_tokens(dreams, test_select) + ops.dream_render -- and the returned action bit for bit that of an engine built with
    dreams=() on the same inputs and noise.  `reset_at`: that step begins with reset(mask) of episode `slot` (its window is padded
    again).  Returns (rows, the dreams of the last step)."""
    from dreamvla_amd import ops
    from dreamvla_amd.rollout import RolloutEngine
    from tests.model_checks import BF, TOL_MODEL, output_tolerances
    from tests.rollout_checks import WindowOracle
    fx, m, (ip, iw, st, tx) = _model(name)
    S, B = fx["S"], episodes
    names = m.dream_names()
    tols = output_tolerances(fx, TOL_MODEL)
    tn = fx["test_noise"].to("cuda")
    steps_a = tn.shape[1]
    every = sample == "all"
    tag = f"dream.engine.{name}.B{B}.graph{int(use_graph)}.{sample}"
    res = []
    with ops.gemm_trials(False):       # the two engines must run the same GEMM configurations: no tuner trials between their captures
        eng = RolloutEngine(m, B, use_graph=use_graph, warmup_decodes=1, sample=sample, dreams=names)
        plain = RolloutEngine(m, B, use_graph=use_graph, warmup_decodes=1, sample=sample)
        g = torch.Generator().manual_seed(41)
        text = torch.randint(1, 49000, (B, 77), generator=g)
        text[:, 24] = 49407
        text[:, 25:] = 0
        text = text.to("cuda")
        text[slot] = tx[0, 0]
        oracle = WindowOracle(S)
        total = S + extra_steps
        for t in range(total):
            k = t % S
            if reset_at is not None and t == reset_at:
                mask = torch.zeros(B, dtype=torch.bool)
                mask[slot] = True
                eng.reset(mask)
                plain.reset(mask)
                oracle = WindowOracle(S)
            if B > 1:
                fp = torch.randn(B, 3, 224, 224, generator=g).to(BF).to("cuda")
                fw = torch.randn(B, 3, 224, 224, generator=g).to(BF).to("cuda")
                fs = torch.rand(B, st.shape[-1], generator=g).to(BF).to("cuda")
                fp[slot], fw[slot], fs[slot] = ip[0, k], iw[0, k], st[0, k]
            else:
                fp, fw, fs = ip[:, k], iw[:, k], st[:, k]
            noise = torch.randn(B * S, steps_a, 7, generator=g).to(BF).float().to("cuda")
            if t == S - 1 and reset_at is None:
                noise.view(B, S, steps_a, 7)[slot] = tn
            action, _, _ = eng.step(fp, fw, fs, text, noise=noise)
            action0, _, _ = plain.step(fp, fw, fs, text, noise=noise)
            res.append(_row(f"{tag}.t{t}.action bit-identical to an engine without dreams", 0, 0, ok=torch.equal(action, action0)))
            got = eng.last_dreams
            res.append(_row(f"{tag}.t{t}.last_dreams holds {sorted(got)}", 0, 0, ok=sorted(got) == sorted(names)))
            window, pick = oracle.push(k)
            if B > 1 and t != total - 1:
                continue                                   # lock-step: the module-level comparison once, on the full window
            # module-level call on the same window of episode `slot`
            with torch.no_grad():
                parts = m.encode_frames(ip[:, window], iw[:, window], st[:, window], tx[:, window])
                sel = torch.tensor([pick], device="cuda")
                ref = m.decode_tokens(parts, mode="test", test_noise=None, test_select=None if every else sel, dreams=names) \
                    if not fx["cfg"]["use_dit_head"] else \
                    m.decode_tokens(parts, mode="test", test_noise=(noise.view(B, S, steps_a, 7)[slot] if every else noise.view(B, S, steps_a, 7)[slot, pick:pick + 1]),
                                    test_select=None if every else sel, dreams=names)
                cur = torch.stack((ip[0, window], iw[0, window]), dim=1)            # (S, 2, 3, h, w)
                if not every:
                    cur = cur[pick:pick + 1]
            for kname in names:
                i = SLOT[kname]
                t_rel, t_abs, _ = tols[i]
                p = ref[i][:, :, 0]                          # (S or 1, 2, rows, cols)
                mine = got[kname][slot]
                if not every:
                    mine = mine.unsqueeze(0)
                if kname == "image":
                    want = ops.dream_render(p.reshape(-1, *p.shape[2:]), "image", cur.reshape(-1, *cur.shape[2:])).view(*p.shape[:2], 224, 224, 3)
                    ok_t = mine.dtype == torch.uint8 and tuple(mine.shape) == tuple(want.shape)
                    worst = float((mine.float() - want.float()).abs().max()) if ok_t else float("inf")
                    res.append(_row(f"{tag}.t{t}.image uint8 {tuple(got[kname].shape)} vs module-level render (max level difference)",
                                    worst, _level_bound(cur, t_abs)))
                elif kname == "depth":
                    want = ops.dream_render(p.reshape(-1, *p.shape[2:]), "depth").view(*p.shape[:2], 224, 224)
                    ok_t = mine.dtype == torch.float32 and tuple(mine.shape) == tuple(want.shape)
                    res.append(dict(_pair(f"{tag}.t{t}.depth float32 {tuple(got[kname].shape)} vs module-level", mine, want, t_rel, t_abs)) if ok_t
                               else _row(f"{tag}.t{t}.depth shape {tuple(mine.shape)}", 0, 0, ok=False))
                else:
                    ok_t = tuple(mine.shape) == tuple(p.shape)
                    res.append(dict(_pair(f"{tag}.t{t}.{kname} {tuple(got[kname].shape)} vs module-level", mine, p, t_rel, t_abs)) if ok_t
                               else _row(f"{tag}.t{t}.{kname} shape {tuple(mine.shape)}", 0, 0, ok=False))
        if use_graph:
            res.append(_row(f"{tag}.graphs captured", 0, 0, ok=eng.graphs_captured))
        if reset_at is None and extra_steps == 0:
            # after the S-th push the window of episode `slot` IS the fixture's: depth / feature dreams of the executed position
            # against the real reference's samples of that position (the image is compared through its prediction in
            # gpu_dream_head_checks: a uint8 frame cannot be turned back into one)
            from tests.model_checks import rel_l2
            for kname in names:
                if kname == "image":
                    continue
                i = SLOT[kname]
                t_rel, t_abs, _ = tols[i]
                rec = fx["train"][i]
                mine = eng.last_dreams[kname][slot]
                if every:
                    mine = mine[S - 1]
                if kname == "depth":
                    mine = patchify(mine.unsqueeze(1), 16)            # (2, 196, 256): back to the head's layout (a permutation)
                per = mine.numel()
                inside = (rec["idx"] >= (S - 1) * per) & (rec["idx"] < S * per)
                gv = mine.float().cpu().flatten()[rec["idx"][inside] - (S - 1) * per]
                wv = rec["vals"][inside]
                r, worst = rel_l2(gv, wv), float((gv - wv).abs().max())
                res.append({"name": f"{tag}.{kname} of the executed position vs the real reference's {int(inside.sum())} samples",
                            "rel_l2": r, "tol": t_rel, "max_abs": worst, "max_abs_tol": t_abs,
                            "ok": bool(int(inside.sum()) > 0 and r <= t_rel and worst <= t_abs)})
    return res, {k: v.clone() for k, v in eng.last_dreams.items()}
