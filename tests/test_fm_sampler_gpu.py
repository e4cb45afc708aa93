"""GPU: the flow-matching head's fused evaluation sampler.
  * dvla_fm_cfg_step (ops.fm_cfg_step) against the ATen guidance + Euler expression it replaces: bit-identical;
  * ActionModelFM.sample_fm_cfg (launch by launch) against FMDiffusion.ddim_sample_loop over forward_with_cfg, both against the
    REAL reference's samples of fixture F;
  * dvla_dit_sample_fm (the whole sampler as one persistent kernel) against the launch-by-launch sampler and the fp32 loop, at
    the bounds tests/gpu_checks.py::check_dit_team holds the DDIM kernel to;
  * the timeout recovery of RolloutEngine on the flow-matching kernel, and fixture F through the engine with its decode graph."""
import pytest
import torch

from tests import gpu_checks as G
from tests import model_checks as C

BF = torch.bfloat16


def _assert_all(results):
    C.report(results)
    bad = [r for r in results if not r["ok"]]
    assert not bad, bad


@pytest.mark.gpu
def test_fm_cfg_step_is_bit_identical_to_the_aten_expression():
    from dreamvla_amd import ops
    g = torch.Generator().manual_seed(9)
    T, C_ = 3, 7
    for bs in (1, 2, 5, 64, 700):
        for pad in (0, 1):                      # model output: the action rows of the (2 bs, [pad +] 2 T, C) DiT output
            for cfg in (1.0, 1.5):
                full = (torch.randn(2 * bs, 2 * T + pad, C_, generator=g) * 2).to(BF).cuda()
                mo = full[:, T + pad:, :]
                x = torch.randn(bs, T, C_, generator=g).cuda()
                delta = 1.0 / 10
                got = ops.fm_cfg_step(mo, x, cfg, delta)
                # DiT.forward_with_cfg's guidance (action_model/models.py) and FMDiffusion's update (gaussian_diffusion.py)
                cond, unc = torch.split(mo, bs, dim=0)
                half = unc + cfg * (cond - unc)
                final = torch.cat([x, x], 0)
                want = (final + delta * torch.cat([half, half], 0).to(final.dtype))[:bs]
                assert torch.equal(got, want), (bs, pad, cfg, float((got - want).abs().max()))


def _fixture_f_model():
    fx = C.load("dreamvla_F.pt")
    m = C.build_hip_model(fx["cfg"]).to(BF).to("cuda")
    m._init_model_type()
    m.eval()
    return fx, m


@pytest.mark.gpu
def test_sample_fm_cfg_vs_op_by_op_loop_on_fixture_f():
    """fixture F (the REAL reference's flow-matching head, its samples from a recorded start noise): the fused sampler
    (ActionModelFM.sample_fm_cfg, launch by launch: all S window positions are sampled) and the operation-by-operation loop
    (`fast_sampler = False`: FMDiffusion over forward_with_cfg) each against the reference's samples, and against each other
    at the bound tests/model_checks.py puts on the DDIM fast path"""
    from dreamvla_amd import ops
    fx, m = _fixture_f_model()
    inp = {k: v.to("cuda") for k, v in C.golden_inputs(fx).items()}
    args = (inp["image_primary"].to(BF), inp["image_wrist"].to(BF), inp["state"].to(BF), inp["text_token"])
    with torch.no_grad():
        parts = m.encode_frames(*args)
        tn = fx["test_noise"].to("cuda")
        calls = {"fm_cfg_step": 0}
        real_step = ops.fm_cfg_step

        def counting(*a, **k):
            calls["fm_cfg_step"] += 1
            return real_step(*a, **k)
        ops.fm_cfg_step = counting
        try:
            out = m.decode_tokens(parts, mode="test", test_noise=tn)
        finally:
            ops.fm_cfg_step = real_step
        m.fast_sampler = False
        try:
            out_slow = m.decode_tokens(parts, mode="test", test_noise=tn)
        finally:
            m.fast_sampler = True
    res = [{"name": f"hip.F fused sampler ran ({calls['fm_cfg_step']} fm_cfg_step launches)", "rel_l2": 0.0, "tol": 0.0,
            "ok": calls["fm_cfg_step"] == 10}]
    rec = ("ref_test_bf16_deviation",)
    res += C.compare_outputs(out, fx["test"], C.TOL_MODEL, "hip.F.test(fused FM sampler)", fx=fx, records=rec)
    res += C.compare_outputs(out_slow, fx["test"], C.TOL_MODEL, "hip.F.test(op-by-op FM sampler)", fx=fx, records=rec)
    dev = fx["ref_test_bf16_deviation"]
    for i, nm in enumerate(("arm", "gripper")):
        r, t = C.rel_l2(out[i], out_slow[i]), 2.0 * C.REF_DEV_FACTOR * dev[i]["rel_l2"]
        res.append({"name": f"hip.F fused FM sampler vs op-by-op loop: {nm}", "rel_l2": r, "tol": t, "ok": r <= t})
    _assert_all(res)


def _fm_loop_fp32(sd32, cond, noise, steps, depth, heads):
    """the flow-matching sampler in fp32 on the CPU (oracle/model_ref.py fm_sample: guidance scale 1, Euler steps of 1 / steps)"""
    from oracle import model_ref
    return model_ref.fm_sample(sd32, "net", cond, torch.cat([noise, noise], 0), steps=steps, depth=depth, heads=heads)


def check_dit_team_fm(bs=1, seeds=(0, 1, 2, 3), fp32_master=False):
    """dvla_dit_sample_fm against the launch-by-launch sampler (sample_fm_cfg with team_sampler = False) and the fp32 loop: the
    bounds of gpu_checks.check_dit_team (deviation 13) -- the persistent kernel at most 1.5 x the launch-by-launch path's
    deviation from the fp32 samples, the two within 2.5 x of it -- bit-reproducible, run on one XCC"""
    from dreamvla_amd import ops
    from dreamvla_amd.action_model.action_model import ActionModelFM
    from oracle import weights
    depth, heads = 12, 12
    am = ActionModelFM(token_size=1024, model_type="DiT-B", in_channels=7, future_action_window_size=2, past_action_window_size=0)
    am.load_state_dict(weights.fill_state_dict(am.state_dict()), strict=True)
    if fp32_master:
        am.load_state_dict({k: (v * 1.0009765625 if v.is_floating_point() else v) for k, v in am.state_dict().items()})
        am = am.to("cuda").eval()
        sd32 = {k: (v.to(BF).float() if v.dim() >= 2 else v.float()).cpu() for k, v in am.state_dict().items()}
    else:
        am = am.to(BF).to("cuda").eval()
        sd32 = {k: v.float().cpu() for k, v in am.state_dict().items()}
    am.create_ddim(10)
    tag = f"dit_team_fm DiT-B bs{bs}" + (" fp32 masters" if fp32_master else "")
    taken = ops.dit_team_ok(768, heads, 7, 3, bs, torch.device("cuda", torch.cuda.current_device()))
    res = [{"name": tag + ": shape taken by the persistent kernel", "rel_l2": 0.0, "tol": 0.0, "ok": bool(taken)}]
    num_t = num_l = num_p = den = 0.0
    worst = 0.0
    for sd in seeds:
        g = torch.Generator().manual_seed(900 + sd)
        cond = G.rnd((bs, 3, 1024), g).to("cuda", BF)
        noise = G.rnd((bs, 3, 7), g).to(BF).float().to("cuda")
        if fp32_master:
            cond = cond.float()
        am.team_sampler, am.team_launches = True, 0
        out_t = am.sample_fm_cfg(cond, noise, 1.5)
        out_t2 = am.sample_fm_cfg(cond, noise, 1.5)
        launched = am.team_launches == 2 and am.team_entry is am._fast_tables[("team_fm", "cuda:%d" % torch.cuda.current_device(), 10)]
        am.team_sampler = False
        out_l = am.sample_fm_cfg(cond, noise, 1.5)
        with torch.no_grad():
            ref = _fm_loop_fp32(sd32, cond.float().cpu(), noise.cpu(), 10, depth, heads)
        if sd == seeds[0]:
            res.append({"name": tag + ": the FM kernel ran, finite, bit-reproducible", "rel_l2": 0.0, "tol": 0.0,
                        "ok": launched and bool(torch.isfinite(out_t).all()) and bool(torch.equal(out_t, out_t2))})
        t, l_ = out_t.float().cpu(), out_l.float().cpu()
        num_t += float(((t - ref) ** 2).sum()); num_l += float(((l_ - ref) ** 2).sum()); num_p += float(((t - l_) ** 2).sum())
        den += float((ref ** 2).sum())
        worst = max(worst, float((t - l_).abs().max()))
    e_t, e_l, e_p = (num_t / den) ** 0.5, (num_l / den) ** 0.5, (num_p / den) ** 0.5
    res.append({"name": tag + f": rel-L2 to the fp32 samples, persistent kernel (launch-by-launch: {e_l:.3e})", "rel_l2": e_t,
                "tol": 1.5 * e_l + 1e-3, "ok": e_t <= 1.5 * e_l + 1e-3})
    res.append({"name": tag + ": persistent kernel vs launch-by-launch", "rel_l2": e_p, "tol": 2.5 * e_l + 1e-3, "max_abs": worst,
                "ok": e_p <= 2.5 * e_l + 1e-3})
    mask = int(getattr(am, "team_xcc_mask", 0))
    res.append({"name": tag + f": team ran on one XCC (mask {mask:#x})", "rel_l2": float(bin(mask).count("1")), "tol": 1.0,
                "ok": bin(mask).count("1") == 1})
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("fp32_master", [False, True])
def test_dit_sample_fm_vs_launch_by_launch(fp32_master):
    _assert_all(check_dit_team_fm(fp32_master=fp32_master))


@pytest.mark.gpu
def test_rollout_engine_recovers_from_a_timeout_of_the_fm_kernel():
    """the timeout contract of deviation 13 on the flow-matching kernel: an injected timeout (eager step, captured graph) ends in
    one fallback to the launch-by-launch sampler and finite actions; a later engine runs the kernel again
    (tests/rollout_checks.py::gpu_team_fallback_check on fixture F, whose head is DiT-B flow matching)"""
    from tests import rollout_checks
    res = rollout_checks.gpu_team_fallback_check("F")
    _assert_all(res)


@pytest.mark.gpu
@pytest.mark.parametrize("sample", ["newest", "all"])
def test_rollout_engine_fm_vs_real_reference(sample):
    """fixture F through RolloutEngine with the decode graph captured: "newest" samples one episode's executed position -- the
    persistent FM kernel inside the graph; "all" samples the S window positions -- sample_fm_cfg launch by launch"""
    from dreamvla_amd import ops
    from tests import rollout_checks
    real_team, real_step = ops.dit_team_sample, ops.fm_cfg_step
    seen = {"team_fm": 0, "fm_cfg_step": 0}

    def team(*a, **k):
        seen["team_fm"] += bool(k.get("fm"))
        return real_team(*a, **k)

    def step(*a, **k):
        seen["fm_cfg_step"] += 1
        return real_step(*a, **k)
    ops.dit_team_sample, ops.fm_cfg_step = team, step
    try:
        res = rollout_checks.gpu_rollout_vs_reference("F", use_graph=True, sample=sample)
    finally:
        ops.dit_team_sample, ops.fm_cfg_step = real_team, real_step
    used = seen["team_fm"] > 0 if sample == "newest" else (seen["fm_cfg_step"] > 0 and seen["team_fm"] == 0)
    res.append({"name": f"rollout.ref.F.{sample}: decoded by the fused FM sampler ({seen})", "rel_l2": 0.0, "tol": 0.0, "ok": used})
    _assert_all(res)
