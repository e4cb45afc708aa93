"""The flow-matching head's evaluation sampler before and after the fused path, with the DDIM head's in the same run.  GPU box only,
not a test.  Per number of episodes (1 and 64; DiT-B, 3 action steps, 10 sampler steps):
  sampler alone, hipGraph replay:  fm_loop_us   = FMDiffusion.ddim_sample_loop over forward_with_cfg (before: op by op)
                                   fm_fused_us  = ActionModelFM.sample_fm_cfg (after: one persistent kernel at one episode,
                                                  launch by launch with dvla_fm_cfg_step otherwise)
                                   ddim_us      = ActionModel.sample_ddim_cfg (the DDIM head's default path)
  control step, RolloutEngine with graphs (BASELINE configs[4] model: S = 10, 24 layers, sample="newest"):
                                   fm_before_ms (model.fast_sampler = False), fm_after_ms, ddim_ms
Prints JSON lines; writes them to --out (default profiles/r07_fm_sampler_perf.jsonl).
    python tests/gpu_fm_sampler_perf.py [--out PATH] [--episodes 1 64]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

BF = torch.bfloat16


def graphed_us(fn, warm=3, n=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def sampler_rows(episodes):
    from dreamvla_amd.action_model.action_model import ActionModel, ActionModelFM
    from oracle import weights
    heads = {}
    for name, cls in (("fm", ActionModelFM), ("ddim", ActionModel)):
        am = cls(token_size=1024, model_type="DiT-B", in_channels=7, future_action_window_size=2, past_action_window_size=0)
        am.load_state_dict(weights.fill_state_dict(am.state_dict()), strict=True)
        am = am.to(BF).to("cuda").eval()
        am.create_ddim(10)
        heads[name] = am
    rows = []
    for bs in episodes:
        g = torch.Generator().manual_seed(bs)
        cond = torch.randn(bs, 3, 1024, generator=g).to("cuda", BF)
        noise = torch.randn(bs, 3, 7, generator=g).to(BF).float().to("cuda")
        fm, dd = heads["fm"], heads["ddim"]
        z = torch.cat([cond, fm.net.z_embedder.uncondition.to(BF).unsqueeze(0).expand(bs, 3, -1)], 0)
        start = torch.cat([noise, noise], 0)
        row = {"what": "sampler alone (hipGraph replay, us)", "episodes": bs, "model": "DiT-B", "steps": 10}
        row["fm_loop_us"] = graphed_us(lambda: fm.ddim_diffusion.ddim_sample_loop(
            fm.net.forward_with_cfg, start.shape, start, clip_denoised=False, model_kwargs=dict(z=z, cfg_scale=1.5),
            device=cond.device, start_noise=start))
        fm.team_launches = 0
        row["fm_fused_us"] = graphed_us(lambda: fm.sample_fm_cfg(cond, noise, 1.5))
        row["fm_fused_took_team_kernel"] = getattr(fm, "team_launches", 0) > 0
        dd.team_launches = 0
        row["ddim_us"] = graphed_us(lambda: dd.sample_ddim_cfg(cond, noise, 1.5))
        row["ddim_took_team_kernel"] = getattr(dd, "team_launches", 0) > 0
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def build_model(use_fm):
    from dreamvla_amd.dreamvla_model import DreamVLA
    cfg = dict(finetune_type="calvin", sequence_length=10, num_resampler_query=16, num_obs_token_per_image=9,
               action_pred_steps=3, transformer_layers=24, hidden_dim=1024, transformer_heads=16, phase="finetune",
               obs_pred=True, depth_pred=True, sam_feat_pred=True, use_dit_head=True, attn_implementation="sdpa", use_fm=use_fm)
    torch.manual_seed(0)
    m = DreamVLA(clip_device="cpu", vit_checkpoint_path=None, **cfg).bfloat16().to("cuda")
    m._init_model_type()
    m.eval()
    return m


def control_step_ms(m, B, steps=20):
    from dreamvla_amd.rollout import RolloutEngine
    g = torch.Generator().manual_seed(B)
    frames = [(torch.randn(B, 3, 224, 224, generator=g).to("cuda", BF), torch.randn(B, 3, 224, 224, generator=g).to("cuda", BF),
               torch.cat([torch.rand(B, 6, generator=g), torch.ones(B, 1)], -1).to("cuda", BF)) for _ in range(4)]
    text = torch.randint(1, 49000, (B, 77), generator=g).to("cuda")
    eng = RolloutEngine(m, B, use_graph=True, warmup_decodes=6)
    for i in range(m.sequence_length + 8):
        eng.step(*frames[i % 4], text)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        eng.step(*frames[i % 4], text)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, eng.graphs_captured, eng._team_sampler_in_use()


def control_rows(episodes):
    rows = []
    fm_model, dd_model = build_model(True), build_model(False)
    for B in episodes:
        row = {"what": "control step (RolloutEngine, graphs, S=10, 24 layers, sample=newest, ms)", "episodes": B}
        fm_model.fast_sampler = False
        row["fm_before_ms"], _, _ = control_step_ms(fm_model, B)
        fm_model.fast_sampler = True
        row["fm_after_ms"], row["graphs_captured"], row["fm_after_team_kernel"] = control_step_ms(fm_model, B)
        row["ddim_ms"], _, row["ddim_team_kernel"] = control_step_ms(dd_model, B)
        row["fm_after_over_ddim"] = row["fm_after_ms"] / row["ddim_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_fm_sampler_perf.jsonl"))
    ap.add_argument("--episodes", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--part", choices=["sampler", "control", "all"], default="all")
    a = ap.parse_args()
    rows = []
    if a.part in ("sampler", "all"):
        rows += sampler_rows(a.episodes)
    if a.part in ("control", "all"):
        rows += control_rows(a.episodes)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.part != "all" else "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
