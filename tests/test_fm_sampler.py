"""CPU: the flow-matching head's fused evaluation sampler -- the host surface (ops.fm_cfg_step, ActionModelFM.sample_fm_cfg, the
binding of dvla_fm_cfg_step / dvla_dit_sample_fm), a float32 restatement of the fused step against the ATen expression it
replaces (DiT.forward_with_cfg's guidance + FMDiffusion's Euler update), and RolloutEngine reading the timeout count of the
exact sampler workspace its decode launched on.  The GPU parity is in tests/test_fm_sampler_gpu.py."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_host_surface_exists():
    from dreamvla_amd import ops
    from dreamvla_amd.action_model import ActionModelFM
    assert callable(ops.fm_cfg_step)
    assert list(inspect.signature(ops.fm_cfg_step).parameters) == ["model_out", "x", "cfg_scale", "delta"]
    assert "fm" in inspect.signature(ops.dit_team_sample).parameters
    assert list(inspect.signature(ActionModelFM.sample_fm_cfg).parameters)[:4] == ["self", "cond", "noise", "cfg_scale"]


def test_binding_of_the_new_entry_points():
    from dreamvla_amd import _lib
    res, args = _lib.SYMBOLS["dvla_fm_cfg_step"]
    assert res is ctypes.c_int and len(args) == 9
    assert [a for a in args[6:8]] == [ctypes.c_float, ctypes.c_float]          # cfg_scale, delta
    res, args = _lib.SYMBOLS["dvla_dit_sample_fm"]
    assert res is ctypes.c_int and args == _lib.SYMBOLS["dvla_dit_sample"][1]   # the same parameter struct as dvla_dit_sample
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvla.h")).read(), flags=re.S)
    assert re.search(r"int dvla_fm_cfg_step\(const void\* model_out, int64_t sample_stride, const float\* x, float\* x_next, "
                     r"int64_t bs, int64_t per_sample,\s+float cfg_scale, float delta, void\* stream\);", txt)
    assert "int dvla_dit_sample_fm(const dvla_dit_sample_params* p, void* stream);" in txt
    assert _lib.ABI_VERSION == 9


def _bf16(a):
    """round-to-nearest-even float32 -> bfloat16 -> float32 (finite values)"""
    u = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _fused_step(mo, x, cfg, delta):
    """what fm_cfg_step_kernel (csrc/elementwise.hip) and the team kernel's step boundary compute, in numpy float32 (every
    operation rounded on its own): the guidance rounded to bf16 after each of its three operations, then x + delta u"""
    bs = x.shape[0]
    cond, unc = mo[:bs].astype(np.float32), mo[bs:].astype(np.float32)
    d = _bf16(cond - unc)
    sd = _bf16(np.float32(cfg) * d)
    u = _bf16(unc + sd)
    return x + np.float32(delta) * u


class _FixedOutputDiT:
    """stands in for DiT inside the REAL DiT.forward_with_cfg: returns the next of the given bf16 model outputs"""

    def __init__(self, outs, in_channels):
        self.outs, self.in_channels, self.k = outs, in_channels, 0

    def forward(self, x, t, z):
        out = self.outs[self.k]
        self.k += 1
        assert x.dtype == torch.bfloat16 and t.dtype == torch.float32
        return out


def test_fused_step_restatement_matches_the_aten_sampler_loop():
    """FMDiffusion.ddim_sample_loop over DiT.forward_with_cfg (the code the fused kernels replace, run here with recorded model
    outputs) against the fused step applied `steps` times: bit-identical, for several batch sizes and guidance scales"""
    from dreamvla_amd.action_model.gaussian_diffusion import FMDiffusion
    from dreamvla_amd.action_model.models import DiT
    g = torch.Generator().manual_seed(3)
    for bs, steps, cfg in ((1, 10, 1.0), (2, 10, 1.5), (5, 7, 1.0), (64, 10, 3.0)):
        T, C = 3, 7
        outs = [(torch.randn(2 * bs, T, C, generator=g) * 2).to(torch.bfloat16) for _ in range(steps)]
        start = torch.randn(bs, T, C, generator=g)
        fake = _FixedOutputDiT(outs, C)
        fd = FMDiffusion(steps)

        def model(x, t, z, cfg_scale):
            return DiT.forward_with_cfg(fake, x, t, z, cfg_scale)
        got = fd.ddim_sample_loop(model, (2 * bs, T, C), None, model_kwargs=dict(z=None, cfg_scale=cfg), device="cpu",
                                  start_noise=torch.cat([start, start], 0))[:bs]
        # FMDiffusion forces the guidance scale to 1.0, whatever the caller passes
        x = start.numpy().astype(np.float32)
        for o in outs:
            x = _fused_step(o.float().numpy(), x, 1.0, 1.0 / steps)
        assert got.dtype == torch.float32
        assert np.array_equal(got.numpy(), x), (bs, steps, float(np.abs(got.numpy() - x).max()))
        # and the guidance at the scale the kernels take as an argument (sample_fm_cfg passes 1.0; the op takes any)
        o = outs[0]
        cond, unc = torch.split(o, bs, dim=0)
        want = (start + (1.0 / steps) * (unc + cfg * (cond - unc)).to(torch.float32)).numpy()
        assert np.array_equal(_fused_step(o.float().numpy(), start.numpy(), cfg, 1.0 / steps), want)


class _Backbone(torch.nn.Module):
    sequence_length = 2
    hidden_dim = 8
    use_dit_head = True

    def __init__(self, am, entry):
        super().__init__()
        self.transformer_backbone = torch.nn.Linear(8, 8)
        self.action_model = am
        self.entry = entry
        self.eval()

    def decode_tokens(self, tokens, mode, test_noise=None, test_select=None):
        # what sample_ddim_cfg / sample_fm_cfg record when they launch the persistent kernel
        self.action_model.team_launches = getattr(self.action_model, "team_launches", 0) + 1
        self.action_model.team_entry = self.entry
        z = torch.zeros(1, 1, 3, 6)
        return (z, z[..., :1])


def test_engine_reads_the_workspace_its_decode_used():
    """round-6 ADVICE: a model that has sampled with two step counts (or with both samplers) holds one workspace per sampler; the
    engine must read the timeout count (word 33) of the one ITS decode launched on -- here the second of two 'team' entries"""
    from dreamvla_amd.rollout import RolloutEngine

    def entry():
        return {"ws": torch.zeros(4096, dtype=torch.uint8), "timeouts": 0}
    am = torch.nn.Module()
    am._fast_tables = {("team", "cpu", 10): entry(), ("team", "cpu", 20): entry(), ("team_fm", "cpu", 10): entry()}
    used = am._fast_tables[("team", "cpu", 20)]
    m = _Backbone(am, used)
    eng = RolloutEngine(m, 1, use_graph=False, sample="newest")
    eng._decode_eager(torch.zeros(1, 2, 36, 8), torch.zeros(1, 3, 7), torch.zeros(1, dtype=torch.long))
    assert eng._team_sampler_in_use()
    assert eng._team_status() is used
    # a timeout counted on ANOTHER workspace is not this engine's ...
    am._fast_tables[("team", "cpu", 10)]["ws"][:384].view(torch.int32)[33] = 1
    assert not eng._team_timed_out()
    # ... one counted on its own is, once
    used["ws"][:384].view(torch.int32)[33] = 1
    assert eng._team_timed_out()
    assert used["timeouts"] == 1 and am._fast_tables[("team", "cpu", 10)]["timeouts"] == 0
    assert not eng._team_timed_out()
    # the flow-matching sampler's workspace, recorded the same way
    m.entry = am._fast_tables[("team_fm", "cpu", 10)]
    eng._decode_eager(torch.zeros(1, 2, 36, 8), torch.zeros(1, 3, 7), torch.zeros(1, dtype=torch.long))
    assert eng._team_status() is m.entry


def test_fm_lookahead_kernel_has_no_spills_and_touches_no_register_in_flight(tmp_path):
    """the flow-matching instantiation of the look-ahead sampler kernel (dit_team_kernel_ahead<3, 1, true>) passes the audit
    tests/test_dit_team_isa.py runs on the DDIM one: no VGPR spills, no register read before its hand-issued load has landed"""
    from tests.probes import isa_inflight_audit as A
    out = tmp_path / "dit_team.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c",
                        os.path.join(ROOT, "dreamvla_amd", "csrc", "dit_team.hip"), "-o", str(out), "-save-temps=obj"],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    listing = open(tmp_path / "dit_team-hip-amdgcn-amd-amdhsa-gfx950.s").read()
    name = "dit_team_kernel_aheadILi3ELi1ELb1EE"
    meta = listing[listing.index("amdhsa.kernels"):]
    mine = [b for b in re.split(r"\n  - ", meta) if name in b and ".vgpr_spill_count" in b]
    assert mine, "kernel metadata not found"
    assert re.search(r"\.vgpr_spill_count:\s+0\b", mine[0]), mine[0][-600:]
    lines = A.function_lines(listing, name)
    flags, nblocks, steps = A.audit(lines)
    assert steps > 5000 and nblocks > 100, (nblocks, steps)
    assert flags == [], flags[:5]
