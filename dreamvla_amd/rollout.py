"""Closed-loop rollout engine: the evaluation-time use of the hot path (BASELINE.json
configs[4]).

The reference evaluates with `ModelWrapper.step` (utils/eval_utils_calvin.py:82-147, same in eval_utils_libero.py):
per control step it appends the newest camera frames / robot state to `history_len`-deep queues, pads a short history
by repeating the last frame, calls `model(..., mode="test")` on the WHOLE window -- re-encoding all `history_len`
frames through the ViT and the resampler although only one of them is new -- and picks the action of the newest real
frame.  This engine keeps that contract (same queue / padding / selection semantics, same DreamVLA weights, batched
over independent episodes) and removes the redundant work:

  * the instruction's text token is computed once per instruction (`text_embedding`), not once per frame and step;
  * per-frame token cache: `DreamVLA.encode_frames` output (text | state | 2 x 16 resampled image tokens | 2 cls tokens
    = 36 x H per frame) of every frame seen so far lives in a (B, S, 36, H) ring in HBM; a control step encodes ONLY
    the newest frame (1/S of the ViT + resampler + CLIP work), shifts the ring and decodes;
  * both halves of a step have static shapes -- the newest-frame encode (CLIP text tower, ViT on two views, resampler,
    projectors) and the decode (token assembly, 24-layer trunk under the block mask, action head incl. the 10-step DDIM
    sampler with classifier-free guidance; the sampler's start noise is a graph INPUT) -- so each is captured once into a hipGraph (`torch.cuda.CUDAGraph`; the
    ctypes kernel launches go to torch's current stream, which is the capture stream) and replayed per step: ~1 700
    kernel launches of a few microseconds each at B = 1 are launch-bound otherwise.

  * dreams (opt-in, `dreams=`; an addition -- the reference decodes them in mode="train" only): the decode also runs the requested
    dream heads on the executed position's query rows, which the trunk computes anyway, and renders them (csrc/dream.hip);
    `last_dreams` holds the frame the policy expects next, its depth map and its feature predictions for every control step.
  * scores of the dreams (opt-in, `score_dreams=`; an addition): `horizon` steps later the predicted frame really arrives; the
    engine keeps both on the device and scores them there (csrc/dream_score.hip), next to the persistence baseline:
    `last_dream_scores`.
  * pictures of the other dreams (opt-in, `dream_views=`; an addition): the same decode turns the depth, trajectory, DINO and SAM
    dreams into uint8 frames (csrc/dream_view.hip: colour-mapped depth, flow wheel, motion mask and its overlay on the current
    frame, features through a fixed palette): `last_dream_views`.

  * attention maps (opt-in, `attention=`; an addition): the newest-frame encode and the decode also report where the selected trunk
    rows -- by default the executed position's action queries -- look (csrc/attention_probe.hip), as further outputs of the same
    graphs; `last_attention` holds the maps, their mass per token group and window step, and a patch heat map per camera.

Episodes of one batch advance in lock-step (one `step` = one control step of every episode); `reset(mask)` restarts
the episodes selected by a boolean mask (their history is cleared, the others keep theirs).
"""
import gc
import warnings

import torch

from . import ops
from .ops import GemmTuner


class _Graphed:
    """fn(*tensors) -> tuple of tensors, static shapes: `warmup` eager calls (the GEMM tuner locks its choices, lazily
    built tables and per-kernel attributes get set up), then one capture into a hipGraph and replays on static buffers."""

    def __init__(self, fn, warmup):
        self.fn, self.warmup = fn, int(warmup)
        self.calls = 0
        self.graph = None
        self.static_in = self.static_out = None

    def __call__(self, *tensors):
        if self.graph is None:
            if self.calls < self.warmup:
                self.calls += 1
                return self.fn(*tensors)
            self.static_in = [t.clone() for t in tensors]
            torch.cuda.synchronize()
            was = GemmTuner.frozen
            GemmTuner.frozen = True                      # no timing events / trials inside the capture
            # The cyclic garbage collector must not run inside the capture: a collected object whose destructor calls into HIP
            # (an event, an older graph, a tensor outside the capture's pool) raises "operation not permitted when stream is
            # capturing" from a destructor, i.e. aborts the process.  Round 6: the full GPU suite died exactly so -- "Fatal Python
            # error: Aborted ... Garbage-collecting" under encode_frames inside this capture -- once a few allocations elsewhere
            # had shifted a generation-2 collection into it.  Collect now, keep the collector off until the capture has ended.
            gc_was = gc.isenabled()
            gc.collect()
            gc.disable()
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self.static_out = self.fn(*self.static_in)
                self.graph = g
            finally:
                GemmTuner.frozen = was
                if gc_was:
                    gc.enable()
        for s, t in zip(self.static_in, tensors):
            s.copy_(t)
        self.graph.replay()
        return tuple(o.clone() for o in self.static_out)


class RolloutEngine:
    def __init__(self, model, batch_size, history_len=None, use_graph=True, warmup_decodes=3, sample="newest", text="latched",
                 dreams=(), score_dreams=False, horizon=3, attention=None, dream_views=None):
        self.model = model.module if hasattr(model, "module") else model
        m = self.model
        if m.training:
            raise ValueError("RolloutEngine drives an eval() model (dropout off), like the reference's evaluation")
        self.B = int(batch_size)
        self.S = int(history_len or m.sequence_length)
        if self.S != m.sequence_length:
            raise ValueError("history_len must equal the model's sequence_length (the attention mask is built for it)")
        p = next(m.transformer_backbone.parameters())
        self.device, self.dtype = p.device, p.dtype
        self.H = m.hidden_dim
        self.tokens = None                      # (B, S, 36, H) ring, oldest frame first
        self.count = torch.zeros(self.B, dtype=torch.long)          # host: frames seen per episode (capped at S)
        self.use_graph = bool(use_graph)
        self.warmup_decodes = int(warmup_decodes)
        self._text_ref = self._text_tok = self._text_emb = None
        self.text_encodes = 0                                             # how often the text tower actually ran
        self.needs_noise = bool(getattr(m, "use_dit_head", False))       # the MLP action head samples nothing
        if sample not in ("newest", "all"):
            raise ValueError('sample: "newest" (the sampler runs on the window position the wrapper executes) or "all"')
        # The reference samples an action for every window position and executes one (eval_utils_calvin.py:141-146).  The
        # sampler's batch elements are independent, so "newest" -- DDIM over B rows instead of B * S -- returns the same
        # executed action from the same noise row; "all" keeps the reference's (B, S, steps, .) action outputs.
        self.sample_all = (sample == "all") or not self.needs_noise
        # Dreams (an addition: the reference decodes them in mode="train" only).  `dreams`: names out of ops.DREAM_KINDS that the
        # model has a head for.  The decode -- eager or the captured graph -- then also runs those heads on the executed position's
        # query rows ("newest"; all S positions with sample="all") and the render kernel (ops.dream_render; the image against the
        # real frame of that position, which the engine keeps next to the token ring: 2 views x 301 KB per episode, x S with
        # "all").  `step` returns what it returns without them; the dreams of the last step are in `last_dreams`.
        from .dreamvla_model import DreamVLA
        self.dreams = DreamVLA._check_dreams(m, dreams)
        self.dreams_all = (sample == "all")
        self.last_dreams = {}
        # Pictures of the depth / trajectory / feature dreams (opt-in, an addition: DESIGN.md section 5 item 26).  `dream_views`:
        # dict(depth=True | dict(lo=, hi=[, palette=, nan_color=]), traj=True | dict(thr=1.0[, tint=, alpha=]), dino=FeaturePalette,
        # sam=FeaturePalette), every key among `dreams`.  The pictures are made by the ops.* functions from the very tensors that
        # `last_dreams` holds, inside the same eager or captured decode, and land in `last_dream_views` (see _render_views).
        # None: no tensors, no launches, the same graphs.
        self.dream_views = self._check_dream_views(dream_views)
        self.last_dream_views = {}
        self._keep_frames = "image" in self.dreams or "traj" in self.dream_views
        self._n_px = 224
        self.last_frames_u8 = None              # step_raw: the resized camera frames of the last step, (B, 2, n_px, n_px, 3) uint8
        self.frames = None                      # newest real frame (B, 2, 3, h, w), or the window's (B, S, 2, 3, h, w) with "all"
        # Scoring the dreams (opt-in, an addition: DESIGN.md section 5 item 18).  The image / depth head predicts the frame `horizon`
        # control steps ahead (the reference's --future_steps; losses.calvin_losses has the same default), so `horizon` steps after
        # a dream was made the engine holds both it and the frame it was a dream of: the dream stored `horizon` steps ago is scored
        # against this step's real frame (ops.image_quality / ops.depth_quality, outside the captured graphs), next to "the frame
        # stays as it was `horizon` steps ago", the predictor a dream has to beat.  `last_dream_scores` holds the result of the last
        # step.  Off: no tensors, no launches, the same graphs.
        self.score_dreams = bool(score_dreams)
        self.horizon = int(horizon)
        self._scored = tuple(k for k in ("image", "depth") if k in self.dreams) if self.score_dreams else ()
        if self.score_dreams:
            if not self._scored:
                raise ValueError('score_dreams: "image" or "depth" must be among `dreams` (feature dreams have no target at evaluation)')
            if sample != "newest":
                raise ValueError('score_dreams needs sample="newest": one dream per control step')
            if int(getattr(m, "pred_num", 1)) != 1:
                raise ValueError("score_dreams needs a model with pred_num == 1")
            if self.horizon < 1:
                raise ValueError("horizon: the number of control steps a dream looks ahead, >= 1")
        # Attention maps (opt-in, an addition: DESIGN.md section 5).  `attention`: None, or the spec of DreamVLA.decode_tokens,
        # dict(rows="action" | "obs" | int (B, R) tensor, layers="all" | "last" | indices); "action" / "obs" mean the queries of the
        # EXECUTED window position, whatever `sample` is: the rows are computed inside the decode from the same device tensor that
        # feeds test_select, so one capture serves every step.  The newest-frame encode then also returns its resampler maps and the
        # decode the trunk maps (further static outputs of the two graphs); `last_attention` is filled per step (see _attend).
        # None: no tensors, no launches, the same graphs.
        self.attention = None
        self.last_attention = {}
        self._res_maps = None                   # resampler maps of the newest frame, (2 B, depth, nq, 196 + nq)
        if attention is not None:
            DreamVLA._attention_probe(m, attention, self.B, self.S, torch.zeros(self.B, dtype=torch.long), "cpu")   # validates
            self.attention = dict(rows=attention.get("rows", "action"), layers=attention.get("layers", "all"))
            if torch.is_tensor(self.attention["rows"]):
                self.attention["rows"] = self.attention["rows"].to(self.device, torch.int32).clone()
            self._groups = DreamVLA.token_groups(m)
        self.since_reset = torch.zeros(self.B, dtype=torch.long)    # host: control steps of each episode since its last reset
        self._score_step = 0                    # control steps scored so far: slot `_score_step % horizon` of the rings is the oldest
        self._dream_ring = self._frame_ring = self._depth_ring = None   # (B, horizon, 2, n, n, 3) uint8 x 2, (B, horizon, 2, n, n) float32
        self.last_dream_scores = {}
        # Instruction text.  "latched" = the wrapper's semantics, literally (eval_utils_calvin.py:109-112: `text_queue` is filled
        # once, when it is empty -- i.e. at the first step after `reset()` -- and kept): an episode's instruction is the one it was
        # given at its first step after a reset; a different `text_token` row later is ignored until the next reset.  "current" =
        # every step conditions the whole window on the row passed to that step (the two agree whenever the caller resets when
        # the instruction changes, as evaluate_sequence does per subtask).  round-4 ADVICE.
        if text not in ("latched", "current"):
            raise ValueError('text: "latched" (kept from the first step after reset(), as ModelWrapper.step) or "current"')
        self.text_mode = text
        self._latched = None
        self._no_noise = torch.zeros(1, device=self.device)
        self._decode_g = _Graphed(self._decode_eager, warmup_decodes) if self.use_graph else None
        self._encode_g = _Graphed(self._encode_eager, warmup_decodes) if self.use_graph else None
        self.team_fallbacks = 0                 # times the one-XCD sampler kernel timed out and the engine fell back (see step)
        # The persistent sampler kernel (dvla_dit_sample) is a property of THIS engine's decode path (round-5 ADVICE): whether the
        # engine allows it (`_team_allowed`: False after a timeout), whether its decode -- eager, or the captured graph -- launched
        # it (`_team_in_decode`, recorded when the decode last ran in Python, i.e. at every eager call and at capture time); the
        # kernel's own timeout count (workspace word 33) is read behind every decode that contains it (`_team_timed_out`).
        self._team_allowed = True
        self._team_in_decode = False
        self._team_seen = None
        self._team_entry = None                 # the sampler cache entry (workspace) the decode's team launch used

    _VIEW_OPTIONS = {"depth": ("lo", "hi", "palette", "nan_color"), "traj": ("thr", "tint", "alpha")}

    def _check_dream_views(self, views):
        """`dream_views` -> {name: options}; the palettes go to the engine's device here, outside any capture"""
        from .dream_view import FeaturePalette, depth_palette
        if views is None:
            return {}
        if not isinstance(views, dict):
            raise ValueError("dream_views: a dict(depth=..., traj=..., dino=..., sam=...) expected")
        out = {}
        for k, v in views.items():
            if k not in ("depth", "traj", "dino", "sam"):
                raise ValueError(f'dream_views: {k!r} is not one of "depth", "traj", "dino", "sam" (the image dream is a frame already)')
            if k not in self.dreams:
                raise ValueError(f"dream_views: {k!r} is not among dreams={self.dreams}")
            if k in ("dino", "sam"):
                if not isinstance(v, FeaturePalette):
                    raise ValueError(f"dream_views[{k!r}]: a FeaturePalette expected (fitted once; see dream_view.FeaturePalette)")
                out[k] = v.to(self.device)
                continue
            if v is True:
                v = {}
            if not isinstance(v, dict) or any(o not in self._VIEW_OPTIONS[k] for o in v):
                raise ValueError(f"dream_views[{k!r}]: True or a dict with keys out of {self._VIEW_OPTIONS[k]}")
            v = dict(v)
            if k == "depth":
                if (v.get("lo") is None) != (v.get("hi") is None):
                    raise ValueError("dream_views['depth']: give both lo and hi, or neither")
                pal = v.get("palette")
                v["palette"] = depth_palette(self.device) if pal is None else pal.to(self.device)
            out[k] = v
        return out

    # ------------------------------------------------------------------------------------------------------------
    def reset(self, mask=None):
        """forget the history of the selected episodes (all when mask is None)"""
        if mask is None:
            self.count.zero_()
            self.since_reset.zero_()            # a dream made before a reset is never scored against a frame after it
        else:
            mask = torch.as_tensor(mask, dtype=torch.bool).cpu()
            self.count[mask] = 0
            self.since_reset[mask] = 0

    def _encode_eager(self, image_primary, image_wrist, state, text_emb):
        m = self.model
        with ops.forward_split_k():
            parts = m.encode_frames(image_primary.unsqueeze(1), image_wrist.unsqueeze(1), state.unsqueeze(1), None,
                                    text_embedding=text_emb.view(text_emb.shape[0], 1, 1, -1),
                                    **({} if self.attention is None else dict(attention=self.attention)))
        if self.attention is None:
            return (torch.cat(parts, dim=2)[:, 0],)
        return (torch.cat(parts, dim=2)[:, 0], m.last_attention["resampler"])

    @torch.no_grad()
    def text_embedding(self, text_token):
        """(B, 77) int64 -> (B, H) text tokens.  The instruction of an episode does not change between control steps, and the
        frozen CLIP tower (12 layers, ~110 launches) gives the same embedding for the same tokens: it is kept and re-used while
        the tokens are the same tensor at the same version, or compare equal (the reference re-encodes the text of all
        `history_len` frames every step, utils/eval_utils_calvin.py:127-134)."""
        ref = self._text_ref
        if ref is not None and ref[0] is text_token and ref[1] == text_token._version:
            return self._text_emb
        tok = text_token.to(self.device)
        if self._text_tok is None or tok.shape != self._text_tok.shape or not bool(torch.equal(tok, self._text_tok)):
            self._text_tok = tok.clone()
            self._text_emb = self.model.encode_text(tok.unsqueeze(1))[:, 0, 0].contiguous()
            self.text_encodes += 1
        self._text_ref = (text_token, text_token._version)
        return self._text_emb

    @torch.no_grad()
    def encode_newest(self, image_primary, image_wrist, state, text_token):
        """(B,3,224,224) x 2, (B,7|8), (B,77) int64 -> (B, 36, H) tokens of the newest frame (state encoders, ViT on both
        views, resampler, projectors: one hipGraph when use_graph; the text token comes from `text_embedding`)"""
        f = self._encode_g if self.use_graph else self._encode_eager
        out = f(image_primary.contiguous(), image_wrist.contiguous(), state.contiguous(), self.text_embedding(text_token))
        if self.attention is not None:
            self._res_maps = out[1]
        return out[0]

    def _push(self, new_tok, new_frames=None):
        """queue semantics of ModelWrapper.step: append; while an episode has seen k < S frames its window is
        [f1 .. fk, fk, ..., fk] (eval_utils_calvin.py:118-126); afterwards the window slides.  `new_frames` (B, 2, 3, h, w), with an
        image dream only: the camera frames the tokens came from, kept for the render (the newest, or the same window with "all")."""
        B, S = self.B, self.S
        keep_window = new_frames is not None and self.dreams_all       # sample="all": the image dream of every position needs its frame
        if new_frames is not None and not keep_window:
            self.frames = new_frames
        if self.tokens is None:
            self.tokens = new_tok.unsqueeze(1).expand(B, S, *new_tok.shape[1:]).contiguous()
            if keep_window:
                self.frames = new_frames.unsqueeze(1).expand(B, S, *new_frames.shape[1:]).contiguous()
            self.count.fill_(1)
            return
        k = self.count                                    # frames seen BEFORE this one
        full = (k >= S)
        if bool(full.all()):
            self.tokens = torch.cat((self.tokens[:, 1:], new_tok.unsqueeze(1)), dim=1)
            if keep_window:
                self.frames = torch.cat((self.frames[:, 1:], new_frames.unsqueeze(1)), dim=1)
        else:
            idx = torch.arange(S).unsqueeze(0).expand(B, S)
            kk = k.unsqueeze(1)
            # source slot for window position j: sliding episodes take j+1 (last <- new); filling episodes keep j < k
            # and take the new frame for every j >= k
            src = torch.where(full.unsqueeze(1), (idx + 1).clamp(max=S), torch.where(idx < kk, idx, torch.full_like(idx, S)))
            ext = torch.cat((self.tokens, new_tok.unsqueeze(1)), dim=1)                  # slot S = the new frame
            gather = src.to(self.device).view(B, S, 1, 1).expand(B, S, *new_tok.shape[1:])
            self.tokens = torch.gather(ext, 1, gather)
            if keep_window:
                ext = torch.cat((self.frames, new_frames.unsqueeze(1)), dim=1)
                self.frames = ext[torch.arange(B, device=self.device).view(B, 1), src.to(self.device)]
        self.count = torch.clamp(k + 1, max=S)

    # ------------------------------------------------------------------------------------------------------------
    def _decode_eager(self, tokens, noise, sel, *more):
        """`more`: the kept camera frames (with an image dream or a trajectory view), then the newest frame's resampler maps (with `attention`)"""
        more = list(more)
        frames = more.pop(0) if self._keep_frames else None
        res_maps = more.pop(0) if self.attention is not None else None
        am = getattr(self.model, "action_model", None)
        shared = getattr(am, "team_sampler", True) if am is not None else True
        before = getattr(am, "team_launches", 0) if am is not None else 0
        if am is not None:
            am.team_sampler = bool(shared) and self._team_allowed      # this engine's choice for the duration of ITS decode only
        extra = {}
        if self.attention is not None:        # the executed position's rows, from `sel` on the device
            rows = self.model._attention_rows(self.attention["rows"], self.B, self.S, sel, tokens.device)
            extra = dict(attention=dict(rows=rows, layers=self.attention["layers"]))
        try:
            with ops.forward_split_k():       # the trunk at one episode: 930 rows, K = 4096 in the MLP down-projection
                if not self.dreams:
                    out = self.model.decode_tokens(tokens, mode="test", test_noise=noise if self.needs_noise else None,
                                                   test_select=None if self.sample_all else sel, **extra)
                else:
                    # (the MLP action head ignores test_select: with it the dream heads run on the executed position only)
                    out = self.model.decode_tokens(tokens, mode="test", test_noise=noise if self.needs_noise else None,
                                                   test_select=None if (self.sample_all and self.dreams_all) else sel,
                                                   dreams=self.dreams, **extra)
        finally:
            if am is not None:
                am.team_sampler = shared
                # (an eager call, or the capture of this engine's graph: what it launched is what its replays launch)
                self._team_in_decode = getattr(am, "team_launches", 0) > before
                if self._team_in_decode:          # the workspace of the launch just made (DDIM or flow matching, any step count)
                    self._team_entry = getattr(am, "team_entry", None)
        maps = () if self.attention is None else self._attend(self.model.last_attention["trunk"], res_maps, sel)
        dreams = self._render(out, frames)
        return (out[0], out[1], *dreams, *self._render_views(dreams, frames), *maps)

    _DREAM_SLOT = {"image": 2, "depth": 6, "traj": 7, "dino": 8, "sam": 9}       # positions in decode_tokens' 10-tuple

    def _render(self, out, frames):
        """the requested heads' predictions of one decode -> what `last_dreams` holds, in the order of `self.dreams`: image uint8
        (B, [S,] views, h, w, 3) rendered against the kept frames, depth float32 (B, [S,] views, h, w), features as they are
        (B, [S,] views, rows, cols); a pred_num axis follows `views` when the model predicts more than one frame"""
        res = []
        lead = (self.B, self.S) if self.dreams_all else (self.B,)
        for name in self.dreams:
            p = out[self._DREAM_SLOT[name]]                       # (B [* S], views, pred_num, rows, cols)
            views, pn = p.shape[1], p.shape[2]
            mid = (views,) if pn == 1 else (views, pn)
            if name in ("image", "depth"):
                cur = None
                if name == "image":
                    cur = frames.reshape(-1, *frames.shape[-3:])
                    if pn > 1:
                        cur = cur.unsqueeze(1).expand(-1, pn, -1, -1, -1).reshape(-1, *frames.shape[-3:])
                r = ops.dream_render(p.reshape(-1, *p.shape[3:]), name, cur, patch=self.model.PATCH_SIZE)
                res.append(r.view(*lead, *mid, *r.shape[1:]))
            else:
                res.append(p.reshape(*lead, *mid, *p.shape[3:]))
        return res

    _TRAJ_VIEW_KEYS = ("flow", "wheel", "mask", "overlay")

    def _render_views(self, dreams, frames):
        """the requested pictures of one decode, from the tensors `last_dreams` will hold (`dreams`, in the order of `self.dreams`),
        flat, in the order of `self.dream_views` -- what `_views_dict` turns into `last_dream_views`:
          "depth"        uint8 (B, [S,] views, [pred_num,] h, w, 3): ops.depth_colorize
          "traj"         {"flow" float32 (.., g f, g f, 2): ops.flow_unshuffle; "wheel" uint8 (.., n, n, 3): ops.flow_wheel at the frame's
                         size; "mask" bool (.., g, g): ops.motion_mask, dilated for view 0 (primary) and not for view 1 (wrist), as
                         losses.calvin_losses' fmask; "overlay" uint8 (.., n, n, 3): ops.motion_overlay on the kept current frame}
          "dino", "sam"  uint8 (.., n, n, 3): ops.feature_render through the palette given"""
        res = []
        n_px = self._n_px                                    # the side of the camera frames of this step
        va = 2 if self.dreams_all else 1                     # the `views` axis of a dream
        for name, opt in self.dream_views.items():
            d = dreams[self.dreams.index(name)]
            if name == "depth":
                res.append(ops.depth_colorize(d, opt.get("lo"), opt.get("hi"), opt["palette"], opt.get("nan_color", (0, 0, 0))))
            elif name == "traj":
                flow = ops.flow_unshuffle(d)
                thr = opt.get("thr", 1.0)
                mask = torch.stack([ops.motion_mask(d.select(va, v), thr, dilate=(v == 0)) for v in range(d.shape[va])], dim=va)
                cur = frames[(slice(None),) * va + (slice(0, d.shape[va]),)]
                pn = mask.dim() - va - 3                     # 1 with a pred_num axis behind `views`
                if pn:
                    cur = cur.unsqueeze(va + 1).expand(*cur.shape[:va + 1], d.shape[va + 1], *cur.shape[va + 1:])
                res += [flow, ops.flow_wheel(flow, n_px), mask,
                        ops.motion_overlay(mask, cur, opt.get("tint", (255, 64, 0)), opt.get("alpha", 96))]
            else:
                res.append(ops.feature_render(d, opt, n_px))
        return res

    def _views_dict(self, flat):
        out, flat = {}, list(flat)
        for name in self.dream_views:
            if name == "traj":
                out[name] = dict(zip(self._TRAJ_VIEW_KEYS, flat[:4]))
                flat = flat[4:]
            else:
                out[name] = flat.pop(0)
        return out

    @property
    def _n_view_tensors(self):
        return sum(4 if k == "traj" else 1 for k in self.dream_views)

    @torch.no_grad()
    def _decode(self, tokens, noise, sel):
        args = (tokens, noise, sel) + ((self.frames,) if self._keep_frames else ())
        if self.attention is not None:
            args += (self._res_maps,)
        return (self._decode_g if self.use_graph else self._decode_eager)(*args)

    def draw_noise(self, generator=None):
        """start noise of the action sampler for one control step, float32 on the device: (B*S, action_pred_steps, 7) -- what
        the reference draws inside forward (dreamvla_model.py:941) -- with sample="all", (B, action_pred_steps, 7) with
        "newest".  It is an INPUT of the captured decode graph (a graph replays its kernels, not its random draws), drawn here
        per step unless the caller passes its own to `step`."""
        m = self.model
        rows = self.B * self.S if self.sample_all else self.B
        return torch.randn(rows, m.action_pred_steps, m.action_model.in_channels, device=self.device, generator=generator)

    @property
    def graphs_captured(self):
        return self.use_graph and self._decode_g.graph is not None and self._encode_g.graph is not None

    @torch.no_grad()
    def step(self, image_primary, image_wrist, state, text_token, noise=None, frames_u8=None, depth_now=None):
        """One control step of every episode.  Returns (action (B, 7) float32 on the device: 6 arm values and the
        gripper command in {-1, +1} as ModelWrapper.step builds it (eval_utils_calvin.py:136-146), arm (B,S,steps,6),
        gripper (B,S,steps,1); with the DiT head and sample="newest" the last two are (B,1,steps,.): the executed position
        only).  `noise`: the DiT sampler's start noise (see draw_noise; a (B*S, steps, 7) draw is accepted with "newest" too --
        the executed position's rows are taken); None = drawn here.
        `text_token`: see `text=` of the constructor -- by default an episode keeps the instruction of its first step after a reset.
        With `dreams=` the dreams of this step are in `self.last_dreams` afterwards (clones: valid until the caller drops them).
        With `score_dreams`: `frames_u8` (B, 2, n, n, 3) uint8 are this step's resized camera frames, view 0 = primary (`step_raw`
        supplies them; required when "image" is scored), `depth_now` (B, 2, n, n) float32 this step's depth maps in the label space
        (what preprocess.preprocess_depth returns; optional: without it this step has no depth entry); the scores of the dreams
        made `horizon` steps ago are in `self.last_dream_scores` afterwards (see `_score`)."""
        if "image" in self._scored and frames_u8 is None:
            raise ValueError("a scoring engine needs this step's uint8 frames: step(..., frames_u8=(B, 2, n, n, 3)) or step_raw")
        if self.text_mode == "latched":
            fresh = (self.count == 0) if self.tokens is not None else torch.ones(self.B, dtype=torch.bool)
            if self._latched is None or bool(fresh.all()):
                self._latched = text_token.to(self.device).clone()
            elif bool(fresh.any()):        # (a new tensor object: text_embedding compares and re-encodes only if a row changed)
                self._latched = torch.where(fresh.to(self.device).view(-1, 1), text_token.to(self.device), self._latched)
            text_token = self._latched
        try:
            out = self._step(image_primary, image_wrist, state, text_token, noise)
        except ops.DitTeamTimeout:
            # an EAGER sampler call (warm-up before the capture, or use_graph=False) noticed the timeout itself; the frame was
            # already pushed: fall back and decode this step again
            self._team_fallback()
            out = self._finish_step(noise)
        if self.score_dreams:
            self._score(frames_u8, depth_now)
        return out

    def _score(self, frames_u8, depth_now):
        """`last_dream_scores` of this step, then this step's dreams (the ones of the decode whose action was returned) and frames
        take the oldest slot of the rings.
          "valid"        bool (B,): the episode has run at least `horizon` steps since its last reset -- a dream of THIS episode
                         exists for this frame
          "image"        {"sse", "mse", "psnr", "ssim"} (B, 2), view 0 = primary: the dream of `horizon` steps ago against the frame now
          "persistence"  the same four for the FRAME of `horizon` steps ago against the frame now
          "depth"        ops.depth_quality's dict, (B, 2); only when `depth_now` was given
        Rows of episodes that are not valid hold NaN, the integer fields -1."""
        h = self.horizon
        slot = self._score_step % h
        valid = (self.since_reset >= h).to(self.device)
        scores = {"valid": valid}

        def masked(d):
            return {k: torch.where(valid.view(-1, 1), v, torch.full_like(v, -1 if v.dtype == torch.int64 else float("nan")))
                    for k, v in d.items()}

        if "image" in self._scored:
            dream = self.last_dreams["image"]
            if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.shape != dream.shape:
                raise ValueError(f"frames_u8: uint8 {tuple(dream.shape)} expected (the layout of last_dreams['image'])")
            frames_u8 = frames_u8.to(self.device)
            if self._dream_ring is None:
                self._dream_ring = torch.zeros((self.B, h, *dream.shape[1:]), dtype=torch.uint8, device=self.device)
                self._frame_ring = torch.zeros_like(self._dream_ring)
            scores["image"] = masked(ops.image_quality(self._dream_ring[:, slot], frames_u8))
            scores["persistence"] = masked(ops.image_quality(self._frame_ring[:, slot], frames_u8))
            self._dream_ring[:, slot] = dream
            self._frame_ring[:, slot] = frames_u8
        if "depth" in self._scored:
            dream = self.last_dreams["depth"]
            if self._depth_ring is None:
                self._depth_ring = torch.zeros((self.B, h, *dream.shape[1:]), dtype=torch.float32, device=self.device)
            if depth_now is not None:
                if not isinstance(depth_now, torch.Tensor) or depth_now.dtype != torch.float32 or depth_now.shape != dream.shape:
                    raise ValueError(f"depth_now: float32 {tuple(dream.shape)} expected (the layout of last_dreams['depth'])")
                scores["depth"] = masked(ops.depth_quality(self._depth_ring[:, slot], depth_now.to(self.device)))
            self._depth_ring[:, slot] = dream
        self.since_reset += 1
        self._score_step += 1
        self.last_dream_scores = scores

    def _raw_to_device(self, frames_u8):
        if not isinstance(frames_u8, torch.Tensor):
            import numpy as np
            frames_u8 = torch.from_numpy(np.ascontiguousarray(frames_u8))
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[0] != self.B or frames_u8.shape[-1] != 3:
            raise TypeError(f"step_raw: uint8 camera frames ({self.B}, h, w, 3) expected")
        if not frames_u8.is_cuda and self.device.type == "cuda":
            frames_u8 = frames_u8.pin_memory()                    # one asynchronous copy per camera, as the collator's
        return frames_u8.to(self.device, non_blocking=True)

    @torch.no_grad()
    def step_raw(self, frames_primary_u8, frames_wrist_u8, state, text_token, noise=None, n_px=224, depth_now=None):
        """`step` from the simulator's raw camera frames: (B, h, w, 3) uint8 per camera, host (numpy array or tensor) or device,
        one size per camera.  Upload, CLIP's bicubic Resize + CenterCrop on the device (preprocess.resize_frames_u8: the bytes
        Pillow produces), ToTensor + Normalize + cast (preprocess.preprocess_frames), then `step`: same return value, and the
        same actions bit for bit as `step` on host-resized frames.  The resized frames of this step stay in
        `self.last_frames_u8` (B, 2, n_px, n_px, 3) uint8 on the device, view 0 = primary, 1 = wrist (the layout of
        `last_dreams["image"]`); a scoring engine (`score_dreams`) takes them from here, and `depth_now` as `step` does."""
        from . import preprocess as P
        u8 = torch.stack((P.resize_frames_u8(self._raw_to_device(frames_primary_u8), n_px),
                          P.resize_frames_u8(self._raw_to_device(frames_wrist_u8), n_px)), dim=1)
        x = P.preprocess_frames(u8)                               # (B, 2, 3, n_px, n_px) bf16
        self.last_frames_u8 = u8
        return self.step(x[:, 0], x[:, 1], state, text_token, noise, frames_u8=u8 if self.score_dreams else None, depth_now=depth_now)

    def _step(self, image_primary, image_wrist, state, text_token, noise):
        dt = self.dtype
        image_primary, image_wrist = image_primary.to(self.device, dt), image_wrist.to(self.device, dt)
        self._n_px = int(image_primary.shape[-1])
        new_tok = self.encode_newest(image_primary, image_wrist, state.to(self.device, dt), text_token.to(self.device))
        self._push(new_tok, torch.stack((image_primary, image_wrist), dim=1) if self._keep_frames else None)
        # the wrapper conditions EVERY frame of the window on the current instruction (eval_utils_calvin.py:127-134 repeat the
        # text over the window), so the text token (slot 0 of a frame's 36) is not history: all S frames carry today's embedding
        self.tokens[:, :, 0] = self._text_emb.to(self.tokens.dtype).unsqueeze(1)
        return self._finish_step(noise)

    def _finish_step(self, noise):
        B, S = self.B, self.S
        sel = (self.count - 1).to(self.device)                               # newest real frame of each episode
        bi = torch.arange(B, device=self.device)
        if not self.needs_noise:
            noise = self._no_noise
        elif noise is None:
            noise = self.draw_noise()
        else:
            noise = noise.to(self.device, torch.float32)
            if not self.sample_all and noise.shape[0] == B * S and S > 1:
                noise = noise.view(B, S, *noise.shape[1:])[bi, sel]
        out = self._decode(self.tokens, noise, sel)
        action, arm, grip = self._actions(out[0], out[1], sel, bi)
        if self._team_sampler_in_use() and self._team_timed_out():
            # The one-XCD sampler kernel (dvla_dit_sample) bounds every wait; on a GPU that other work keeps busy its 32 workgroups
            # may not be co-resident, a wait times out and the kernel returns NaN by design.  Under hipGraph replay no Python runs
            # inside the sampler, so the check is HERE, before the action is handed to the environment (round-4 ADVICE: a NaN arm
            # command with gripper -1 went straight out): the kernel's own timeout count (workspace word 33, one 4-byte host read
            # per step on the single-episode path, whose caller reads the action next anyway) against the count this engine last
            # saw -- not "the action is not finite" (round-5 ADVICE: a NaN from a bad observation or bad weights is not a sampler
            # timeout and must not switch the sampler).  Recovery: the launch-by-launch sampler (same arithmetic) for THIS engine,
            # its decode graph re-captured, this step's action recomputed from the same tokens and noise.
            self._team_fallback()
            out = self._decode(self.tokens, noise, sel)
            action, arm, grip = self._actions(out[0], out[1], sel, bi)
        # the dreams of the decode whose action is returned (after a fallback: of the recomputed one)
        self.last_dreams = dict(zip(self.dreams, out[2:2 + len(self.dreams)]))
        if self.dream_views:
            first = 2 + len(self.dreams)
            self.last_dream_views = self._views_dict(out[first:first + self._n_view_tensors])
        if self.attention is not None:
            # `last_attention` of this step (of the decode whose action was returned):
            #   "trunk"   (B, n_layers, R, L) fp32: the head-mean attention of the selected rows in the selected trunk layers
            #   "mass"    (B, R, S, n_groups): its share per token group and window step, averaged over the layers; "groups": the names
            #   "heat"    (B, 2, g, g): ops.patch_heat for the executed position's frame -- the newest real frame, whose resampler
            #             maps ("resampler", (2 B, depth, nq, patches + nq)) the encode of this step produced
            trunk, mass, heat = out[-3:]
            self.last_attention = {"trunk": trunk, "mass": mass, "heat": heat, "groups": [g[0] for g in self._groups],
                                   "resampler": self._res_maps}
        return action, arm, grip

    def _attend(self, trunk, res_maps, sel):
        """what the decode -- eager or the captured graph -- returns next to the actions: the trunk maps, their mass per token group
        and window step, and the patch heat of the executed position's frame (small torch arithmetic, part of the same graph)"""
        return (trunk, ops.attention_mass(trunk, self._groups, self.S).mean(dim=1),
                ops.patch_heat(trunk, res_maps, self._groups, sel))

    def _actions(self, arm, grip, sel, bi):
        B, S = self.B, self.S
        if arm.dim() == 4 and arm.shape[0] == 1 and B * S == arm.shape[1] and self.sample_all:   # DiT test head returns (1, B*S, steps, .)
            arm, grip = arm.view(B, S, *arm.shape[2:]), grip.view(B, S, *grip.shape[2:])
        elif arm.dim() == 4 and arm.shape[0] == 1 and not self.sample_all:                        # (1, B, steps, .)
            arm, grip = arm.view(B, 1, *arm.shape[2:]), grip.view(B, 1, *grip.shape[2:])
        if not self.sample_all:
            sel = torch.zeros_like(sel)
        a = arm[bi, sel, 0, :].float()
        g = (grip[bi, sel, 0, :].float() > 0.5).float()
        return torch.cat((a, (g - 0.5) * 2), dim=-1), arm, grip

    def _team_sampler_in_use(self):
        """did THIS engine's decode path (eager, or its captured graph) launch the persistent sampler kernel?  Recorded by
        `_decode_eager` whenever the decode runs in Python (`ActionModel.sample_ddim_cfg` and `ActionModelFM.sample_fm_cfg` count
        their team launches; the shapes that take the kernel are decided there: one episode, DiT-B)"""
        return bool(self.needs_noise and self._team_in_decode)

    def _team_status(self):
        """the action model's sampler cache entry -- workspace, last timeout count seen -- that THIS engine's decode launched the
        kernel on (recorded by `_decode_eager`; None before the first team launch).  Not a lookup by device: a model that has
        sampled with two timestep counts, or with both samplers, has one workspace each (round-6 ADVICE)."""
        return self._team_entry

    def _team_timed_out(self):
        """has the kernel's timeout count (word 33 of its workspace: include/dvla.h) moved since this engine last looked?"""
        st = self._team_status()
        if st is None:
            return False
        # st["timeouts"] = the count last seen on this workspace by ANYONE (this engine, another engine on the same model, an eager
        # sampler call): the host drives one launch / replay at a time and looks right behind it, so whatever the count moved by
        # since the last look belongs to the replay that has just run
        now = ops.dit_team_status(st["ws"])[0]
        seen = st["timeouts"]
        self._team_seen = st["timeouts"] = now
        return now != seen

    def _team_fallback(self):
        self._team_allowed = False
        self._team_in_decode = False
        self.team_fallbacks += 1
        if self.use_graph:                       # the captured decode contains the team kernel: warm up and capture again
            self._decode_g = _Graphed(self._decode_eager, self.warmup_decodes)
        warnings.warn("RolloutEngine: the one-XCD sampler kernel timed out (the GPU is shared or busy: its 32 workgroups were not co-resident); "
                      "this engine now runs the launch-by-launch sampler", RuntimeWarning)


class TemporalEnsembler:
    """The LIBERO wrapper's temporal ensembling of the action chunk (utils/eval_utils_libero.py:160-176, `use_ensembling`), batched
    over the engine's episodes and kept on the device.

    The reference keeps `all_time_actions` (max_steps, max_steps + action_pred_steps, 7), writes the chunk predicted at control step
    t for the selected window position -- (action_pred_steps, 7): arm (6) and the RAW gripper output -- into row t, columns
    t .. t + action_pred_steps - 1, takes column t of every row whose 7 values are all non-zero (the predictions made for time t at
    steps t - action_pred_steps + 1 .. t, oldest first), averages them with weights exp(-k i) / sum (i = 0 for the OLDEST, k =
    `ensembling_temp`), thresholds the averaged gripper value at 0.5 and maps it to {-1, +1}.  Only the last action_pred_steps rows can
    be populated at column t, so a ring of that many chunks per episode holds the same information as the (max_steps, ...) table.

    `ens = TemporalEnsembler(B, action_pred_steps, temp, device)`; per control step, with sample="newest" outputs of
    `RolloutEngine.step`: `action = ens(arm[:, 0], grip[:, 0])` -> (B, 7) float32; `ens.reset(mask)` with the engine's reset."""

    def __init__(self, episodes, action_pred_steps, temp, device):
        self.B, self.P, self.k = int(episodes), int(action_pred_steps), float(temp)
        self.device = device
        # ring[b, j] = the chunk predicted j control steps ago (j = 0: this step); age[b] = chunks stored so far (capped at P)
        self.ring = torch.zeros(self.B, self.P, self.P, 7, dtype=torch.float32, device=device)
        self.age = torch.zeros(self.B, dtype=torch.long, device=device)
        # weights[n, i]: the reference's float64 numpy weights for n populated rows (:170-172), i = 0 the oldest; row 0 unused
        import numpy as np
        tab = np.zeros((self.P + 1, self.P), dtype=np.float64)
        for n in range(1, self.P + 1):
            e = np.exp(-self.k * np.arange(n))
            tab[n, :n] = e / e.sum()
        self.weights = torch.from_numpy(tab).to(device)

    def reset(self, mask=None):
        if mask is None:
            self.ring.zero_()
            self.age.zero_()
        else:
            m = torch.as_tensor(mask, dtype=torch.bool, device=self.device)
            self.ring[m] = 0
            self.age[m] = 0

    @torch.no_grad()
    def __call__(self, arm, grip):
        """arm (B, action_pred_steps, 6), grip (B, action_pred_steps, 1) of the executed window position -> (B, 7)"""
        B, P = self.B, self.P
        chunk = torch.cat((arm.float(), grip.float()), dim=-1).to(self.device)                  # eval_utils_libero.py:165
        self.ring = torch.roll(self.ring, 1, dims=1)
        self.ring[:, 0] = chunk
        self.age = torch.clamp(self.age + 1, max=P)
        # the prediction for NOW made j steps ago is element j of that chunk; rows older than the episode are absent, and the reference
        # also drops a row whose seven values are not all non-zero (`actions_populated`, :168-169)
        j = torch.arange(P, device=self.device)
        cand = self.ring[:, j, j]                                                               # (B, P, 7), newest first
        have = (j.unsqueeze(0) < self.age.unsqueeze(1)) & (cand != 0).all(dim=-1)
        # weights exp(-k i) with i counted from the OLDEST populated row (:171): rank among the populated ones, oldest = 0
        have_o = torch.flip(have, dims=[1])                                                     # oldest first
        order = (have_o.long().cumsum(1) - 1).clamp_min(0)
        n = have_o.long().sum(1)
        w = self.weights[n.unsqueeze(1), order] * have_o                                        # float64, zero where no row
        # (the reference multiplies float32 actions by float64 weights: product and sum in float64, oldest row first; the absent
        #  rows add exact zeros)
        avg = (torch.flip(cand, dims=[1]).double() * w.unsqueeze(-1)).sum(dim=1)
        g = (avg[:, 6:] > 0.5).to(torch.float32)                                                # :174-175
        return torch.cat((avg[:, :6].to(torch.float32), (g - 0.5) * 2), dim=-1)
