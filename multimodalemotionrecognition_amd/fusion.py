"""``FusionModel`` and friends -- drop-in mirror of ``src/models/fusion.py`` on the MI355X kernels.

Same class names, constructor keyword arguments, module attribute names (hence state-dict
keys: reference checkpoints load unchanged) and forward signatures as the reference
(``fusion.py:11-437``).  The math runs in ``libmer_hip.so``: the xattn head through the
explicit schedule in ``xattn_head.py`` (one autograd node), the concat / gated / late heads
through ``embedding_head.py``.  There is no CPU path: calling the model on CPU tensors raises.
"""
from __future__ import annotations

import dataclasses
import math
import os
import random
from typing import Optional

import torch
from torch import nn

from . import embedding_head as EH
from . import graphs as G
from . import kernels as K
from . import xattn_fused as XF
from . import xattn_head as XH
from .nn_ops import hip_linear
from .temporal import TemporalPooler


def _require_device(*ts):
    for t in ts:
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise RuntimeError("multimodalemotionrecognition_amd runs on MI355X (HIP) only; move the model and "
                               "inputs to a 'cuda' device (the CPU reference lives in oracle/, test-only)")


_SIDE_STREAMS = {}


def _side_stream(device: torch.device):
    """One side stream per device for the audio encoder (created lazily, reused every step)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    s = _SIDE_STREAMS.get(idx)
    if s is None:
        s = _SIDE_STREAMS[idx] = torch.cuda.Stream(device=idx)
    return s


def _next_seed() -> int:
    # host-side draw so that torch.manual_seed() makes runs reproducible (train.py:951 set_seed)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class StochasticDepth(nn.Module):
    """Per-sample drop-path (fusion.py:11-26); applied inside the fused residual+LayerNorm kernel."""

    def __init__(self, drop_prob: float = 0.0) -> None:
        super().__init__()
        self.drop_prob = float(max(0.0, min(1.0, drop_prob)))


class ModalityDropout(nn.Module):
    """Batch-wide modality dropout (fusion.py:29-55): one host draw per modality per batch."""

    def __init__(self, audio_dropout_p: float = 0.2, video_dropout_p: float = 0.2):
        super().__init__()
        self.audio_dropout_p = audio_dropout_p
        self.video_dropout_p = video_dropout_p

    def draw(self):
        if not self.training:
            return False, False
        return (torch.rand(1).item() < self.audio_dropout_p, torch.rand(1).item() < self.video_dropout_p)


class _ClipLossFn(torch.autograd.Function):
    """Symmetric CLIP loss of fusion.py:141-149 on csrc/align.hip (one workgroup, exact fp32)."""

    @staticmethod
    def forward(ctx, a_al, v_al, logit_scale):
        a_al, v_al = a_al.contiguous().float(), v_al.contiguous().float()
        B, D = a_al.shape
        an, vn = torch.empty_like(a_al), torch.empty_like(v_al)
        norms = torch.empty(2 * B, device=a_al.device, dtype=torch.float32)
        logits = torch.empty(B, B, device=a_al.device, dtype=torch.float32)
        loss = torch.empty((), device=a_al.device, dtype=torch.float32)
        K.clip_align_fwd(a_al, v_al, logit_scale.detach().reshape(1), an, vn, norms, logits, loss)
        ctx.sv = (an, vn, norms, logits)
        ctx.logit_scale = logit_scale
        return loss

    @staticmethod
    def backward(ctx, dloss):
        an, vn, norms, logits = ctx.sv
        da, dv = torch.empty_like(an), torch.empty_like(vn)
        ls = ctx.logit_scale
        dls = grad_buffer(ls) if ctx.needs_input_grad[2] else None
        K.clip_align_bwd(an, vn, norms, logits, ls.detach().reshape(1), dloss.contiguous().float().reshape(1), da, dv,
                         dls.view(1) if dls is not None else None)
        return da, dv, dls


class ClipStyleAlignment(nn.Module):
    """fusion.py:127-150: project audio / video embeddings into a shared space + symmetric CLIP loss."""

    def __init__(self, audio_dim: int, video_dim: int, align_dim: int, init_temperature: float = 0.07) -> None:
        super().__init__()
        self.audio_proj = nn.Linear(audio_dim, align_dim)
        self.video_proj = nn.Linear(video_dim, align_dim)
        safe_temp = max(float(init_temperature), 1e-3)
        self.logit_scale = nn.Parameter(torch.tensor(math.log(1.0 / safe_temp), dtype=torch.float32))

    def forward(self, audio_emb: torch.Tensor, video_emb: torch.Tensor):
        """-> (a_aligned, v_aligned, loss), as fusion.py:137-150."""
        _require_device(audio_emb, video_emb)
        a_aligned = hip_linear(audio_emb, self.audio_proj)
        v_aligned = hip_linear(video_emb, self.video_proj)
        return a_aligned, v_aligned, _ClipLossFn.apply(a_aligned, v_aligned, self.logit_scale)


class EmotionPriorBiasAdapter(nn.Module):
    """fusion.py:153-184 (parameters; the math is fused into the xattn head schedule)."""

    def __init__(self, token_dim: int, prior_dim: int, hidden_dim: int, dropout: float = 0.1) -> None:
        super().__init__()
        self.prior_net = nn.Sequential(nn.Linear(token_dim * 2, hidden_dim), nn.ReLU(inplace=True),
                                       nn.Dropout(dropout), nn.Linear(hidden_dim, prior_dim))
        self.v_query_bias = nn.Linear(token_dim + prior_dim, 1)
        self.a_key_bias = nn.Linear(token_dim + prior_dim, 1)
        self.a_query_bias = nn.Linear(token_dim + prior_dim, 1)
        self.v_key_bias = nn.Linear(token_dim + prior_dim, 1)
        self.bias_scale = nn.Parameter(torch.tensor(1.0, dtype=torch.float32))
        self.dropout = float(dropout)


def grad_buffer(param: torch.Tensor) -> torch.Tensor:
    """Where a backward kernel should accumulate ``param``'s gradient.

    When a ``FusedAdam`` owns the parameter and ``param.grad`` is unset, this is the param's
    zeroed view into the optimizer's flat gradient buffer (autograd then adopts it without a
    copy); otherwise a fresh zero buffer (autograd accumulates it into an existing ``.grad``).
    """
    slot = getattr(param, "_mer_grad_slot", None)
    if slot is not None and param.grad is None:
        flat, off = slot
        return flat.narrow(0, off, param.numel()).view(param.shape)  # zeroed by FusedAdam.zero_grad
    return torch.zeros_like(param, dtype=torch.float32)


def _head_grads(p, used):
    grads = {}
    for n, t in p.items():
        if n in used and t.requires_grad:
            grads[n] = grad_buffer(t)
        elif n in used:
            grads[n] = torch.zeros_like(t)
    return grads


class _XattnHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v_feat, a_seq, cfg, training, rng, names, runner, *params):
        p = dict(zip(names, params))
        if runner is not None:
            logits, hctx = runner.forward(v_feat, a_seq)
            ctx.gen = runner.cur_gen
            ctx.token = runner.token(ctx.gen)
        else:
            logits, hctx = XH.head_forward(p, cfg, v_feat, a_seq, training, rng)
        ctx.hctx, ctx.names, ctx.params, ctx.runner = hctx, names, params, runner
        ctx.used = set(XH.used_param_names(cfg))
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        p = dict(zip(ctx.names, ctx.params))
        dl = dlogits.contiguous().float()
        need_v = ctx.needs_input_grad[0]
        need_a = ctx.needs_input_grad[1]
        if ctx.runner is not None and ctx.runner.backward_graphable(p, ctx.used, need_v, need_a):
            dv, grads = ctx.runner.backward(dl)
            da = None
        else:
            grads = _head_grads(p, ctx.used)
            dv, da = XH.head_backward(p, ctx.hctx, dl, grads, need_dv_feat=need_v, need_da_seq=need_a)
        if ctx.runner is not None:
            ctx.runner.release(ctx.gen)
        out_grads = [grads.get(n) if (n in ctx.used and t.requires_grad) else None for n, t in p.items()]
        return (dv, da, None, None, None, None, None, *out_grads)


class HeadProbe:
    """bench.py's second roofline entry: HIP events around the xattn head's forward / backward graph replays
    (on the stream they replay on), collected while ``fusion.HEAD_PROBE`` is set."""

    def __init__(self):
        self.fwd, self.bwd = [], []
        self.saved_bytes = 0

    def mark(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def avg_ms(self):
        f = [a.elapsed_time(b) for a, b in self.fwd]
        b = [a.elapsed_time(c) for a, c in self.bwd]
        if not f or not b:
            return None
        return sum(f) / len(f), sum(b) / len(b)


HEAD_PROBE = None


class _HeadGraphs(G.PendingGuard):
    """Captured forward / backward hipGraphs of the xattn head for one input shape (graphs.py).

    The dropout / drop-path masks stay random per step: the graph's RNG base is a static device scalar that
    is refilled with the step's host-drawn seed right before each replay (so ``torch.manual_seed`` fixes
    the masks exactly as in eager mode), and the backward graph regenerates the same masks from it.
    ``pending`` marks a forward whose backward has not run yet: a second forward in between (gradient
    accumulation) runs eagerly instead of overwriting the saved static activations.
    """

    def __init__(self, model, names, cfg, training):
        super().__init__()
        self.model, self.names, self.cfg, self.training = model, names, cfg, training
        self.fwd = self.bwd = None
        self.cur_gen = 0
        self.rng = None

    def forward(self, v_feat, a_seq):
        params = dict(zip(self.names, self.model.head_params()[1]))
        if self.fwd is None:
            if XF.supported(self.cfg, params, v_feat, a_seq, None):
                XF.planes_for(params)  # host-side setup (an H2D descriptor copy) outside the capture
            self.rng = torch.zeros(1, dtype=torch.int64, device=v_feat.device)
            self.fwd = G.StaticGraph(lambda v, a: XH.head_forward(params, self.cfg, v, a, self.training,
                                                                  self.rng if self.training else None),
                                     [v_feat, a_seq])
        if self.training:  # this step's host-drawn RNG base, stream-ordered before the replay reads it
            self.rng.fill_(self.model.take_head_seed())
        probe = HEAD_PROBE
        e0 = probe.mark() if probe is not None else None
        logits, hctx = self.fwd.replay(v_feat, a_seq)
        if probe is not None:
            probe.fwd.append((e0, probe.mark()))
            probe.saved_bytes = sum(t.numel() * t.element_size() for t in hctx.saved.values())
        return logits.clone(), hctx

    def backward_graphable(self, p, used, need_v, need_a) -> bool:
        return (not need_a) and all(t.grad is None and getattr(t, "_mer_grad_slot", None) is not None
                                    for n, t in p.items() if n in used and t.requires_grad)

    def backward(self, dlogits):
        params = dict(zip(self.names, self.model.head_params()[1]))
        used = set(XH.used_param_names(self.cfg))
        if self.bwd is None:
            _, hctx = self.fwd.out

            def run(dl):
                grads = _head_grads(params, used)
                dv, _ = XH.head_backward(params, hctx, dl, grads, need_dv_feat=True, need_da_seq=False)
                return dv

            self.bwd = G.StaticGraph(run, [dlogits])
        probe = HEAD_PROBE
        e0 = probe.mark() if probe is not None else None
        dv = self.bwd.replay(dlogits)
        if probe is not None:
            probe.bwd.append((e0, probe.mark()))
        # dv goes straight back through autograd into the trunk backward of this same pass, before the next
        # replay of this graph: the static tensor itself, no copy
        return dv, {n: grad_buffer(t) for n, t in params.items() if n in used and t.requires_grad}


class FusionModel(nn.Module):
    def __init__(
        self,
        audio_model: nn.Module,
        video_model: nn.Module,
        num_classes: int,
        mode: str = "late",
        common_dim: int = 256,
        xattn_head: str = "concat",
        d_model: int = 128,
        num_heads: int = 4,
        audio_n_mels: int = 64,
        xattn_attn_dropout: float = 0.1,
        xattn_stochastic_depth: float = 0.1,
        temporal_pooling: str = "mean",
        temporal_num_heads: int = 4,
        temporal_num_layers: int = 1,
        temporal_dropout: float = 0.1,
        fusion_align_mode: str = "none",
        fusion_align_dim: int = 256,
        fusion_align_temperature: float = 0.07,
        xattn_use_emotion_prior: bool = False,
        xattn_emotion_prior_dim: int = 8,
        xattn_emotion_prior_hidden_dim: int = 64,
        xattn_emotion_prior_dropout: float = 0.1,
    ) -> None:
        super().__init__()
        self.audio_model = audio_model
        self.video_model = video_model
        self.mode = mode
        self.d_model = d_model
        self.num_heads = num_heads
        self.audio_n_mels = audio_n_mels
        self.fusion_align_mode = fusion_align_mode
        self.alignment_loss = None
        self.semantic_alignment = None
        self.xattn_use_emotion_prior = xattn_use_emotion_prior
        self.num_classes = num_classes
        self._prefetched = None  # (audio key, encoder output, stream) from prefetch_audio()
        self._queued_audio = None  # the NEXT batch's waveform for an early prefetch (queue_next_audio)
        self._head_seed = None  # this forward's head dropout seed, drawn ahead of an early prefetch
        self._head_graphs = G.GraphCache()

        if mode in {"concat", "gated"}:
            fusion_audio_dim = audio_model.embedding_dim
            fusion_video_dim = video_model.embedding_dim
            if fusion_align_mode == "clip":
                self.semantic_alignment = ClipStyleAlignment(audio_model.embedding_dim, video_model.embedding_dim,
                                                             fusion_align_dim, fusion_align_temperature)
                fusion_audio_dim = fusion_video_dim = fusion_align_dim
            self.audio_proj = nn.Linear(fusion_audio_dim, common_dim)
            self.video_proj = nn.Linear(fusion_video_dim, common_dim)
            if mode == "concat":
                self.fusion = nn.Sequential(nn.Linear(common_dim * 2, common_dim), nn.ReLU(inplace=True),
                                            nn.Dropout(0.2), nn.Linear(common_dim, num_classes))
            else:
                self.modality_dropout = ModalityDropout(audio_dropout_p=0.2, video_dropout_p=0.2)
                self.gate = nn.Sequential(nn.Linear(common_dim * 2, common_dim), nn.ReLU(inplace=True),
                                          nn.Dropout(0.2), nn.Linear(common_dim, 1), nn.Sigmoid())
                self.classifier = nn.Linear(common_dim, num_classes)
                with torch.no_grad():  # fusion.py:329-336: both gate Linear biases become -1
                    self.gate[0].bias.fill_(-1.0)
                    self.gate[3].bias.fill_(-1.0)

        if mode in {"xattn", "xattn_concat", "xattn_gated"}:
            self.v_dim = getattr(video_model, "embedding_dim", 512)
            self.audio_sequence_dim = getattr(audio_model, "sequence_dim", d_model)
            self.a_dim = d_model
            self.v_in_proj = nn.Linear(self.v_dim, d_model)
            self.a_in_proj = nn.Linear(self.a_dim, d_model)
            # dead on the WavLM path but checkpointed (fusion.py:273)
            self.audio_time_conv = nn.Conv1d(audio_n_mels, self.a_dim, kernel_size=3, padding=1)
            self.audio_seq_proj = nn.Linear(self.audio_sequence_dim, self.a_dim)
            self.v2a_attn = nn.MultiheadAttention(d_model, num_heads, dropout=xattn_attn_dropout, batch_first=True)
            self.a2v_attn = nn.MultiheadAttention(d_model, num_heads, dropout=xattn_attn_dropout, batch_first=True)
            self.v_drop_path = StochasticDepth(drop_prob=xattn_stochastic_depth)
            self.a_drop_path = StochasticDepth(drop_prob=xattn_stochastic_depth)
            self.v_norm = nn.LayerNorm(d_model)
            self.a_norm = nn.LayerNorm(d_model)
            if xattn_use_emotion_prior:
                self.emotion_prior_bias = EmotionPriorBiasAdapter(d_model, xattn_emotion_prior_dim,
                                                                  xattn_emotion_prior_hidden_dim,
                                                                  xattn_emotion_prior_dropout)
            else:
                self.emotion_prior_bias = None
            self.v_temporal_pool = TemporalPooler(d_model, temporal_pooling, temporal_num_heads,
                                                  temporal_num_layers, temporal_dropout)
            self.a_temporal_pool = TemporalPooler(d_model, temporal_pooling, temporal_num_heads,
                                                  temporal_num_layers, temporal_dropout)
            self.xattn_head = xattn_head
            self.attn_dropout = float(xattn_attn_dropout)
            self.temporal_pooling = temporal_pooling
            self.temporal_num_heads = temporal_num_heads
            self.temporal_num_layers = temporal_num_layers
            self.temporal_dropout = float(temporal_dropout)
            if xattn_head == "concat":
                self.xattn_mlp = nn.Sequential(nn.Linear(d_model * 2, common_dim), nn.ReLU(inplace=True),
                                               nn.Dropout(0.2), nn.Linear(common_dim, num_classes))
            elif xattn_head == "gated":
                self.xattn_gate = nn.Sequential(nn.Linear(d_model * 2, d_model), nn.ReLU(inplace=True),
                                                nn.Dropout(0.2), nn.Linear(d_model, 1), nn.Sigmoid())
                self.xattn_classifier = nn.Linear(d_model, num_classes)
                with torch.no_grad():  # fusion.py:338-344: BOTH gate Linear biases become -1
                    self.xattn_gate[0].bias.fill_(-1.0)
                    self.xattn_gate[3].bias.fill_(-1.0)

    def step_rng(self, device) -> torch.Tensor:
        """This step's dropout RNG base: a fresh device int64 [1] tensor drawn from the host generator each
        training forward (so ``torch.manual_seed`` reproduces the masks, train.py:951 set_seed); the
        autograd context keeps it, so masks are regenerated correctly even with several forwards in flight."""
        return torch.full((1,), self.take_head_seed(), dtype=torch.int64, device=device)

    def take_head_seed(self) -> int:
        """The head's dropout seed of this forward: pre-drawn by an early prefetch (``_issue_queued``, which keeps
        the host draw order of the inline schedule -- this step's head, then the next batch's encoder), else drawn
        now."""
        s, self._head_seed = self._head_seed, None
        return _next_seed() if s is None else s

    def audio_encoder_frozen(self) -> bool:
        enc = getattr(self.audio_model, "wavlm", None)
        return enc is not None and not enc.trainable()

    def prefetch_audio(self, audio: torch.Tensor) -> bool:
        """Start the frozen audio encoder on the NEXT batch's waveform, on the side stream, so it runs
        concurrently with this step's backward (the encoder's output does not depend on the weights the
        step updates).  The next ``forward`` whose ``audio`` is this same tensor (same storage, shape and
        version) consumes the result; any other input runs the encoder inline as usual.  Returns whether
        the prefetch was issued (xattn mode with a frozen WavLM encoder only)."""
        xattn = self.mode in {"xattn", "xattn_concat", "xattn_gated"}
        frozen = self.audio_encoder_frozen()
        stage2 = (xattn and not frozen and hasattr(self.audio_model, "encode_prefix") and torch.is_grad_enabled()
                  and getattr(self.audio_model, "wavlm", None) is not None)
        if not (frozen or stage2) or self.mode not in {"xattn", "xattn_concat", "xattn_gated", "late", "concat",
                                                       "gated"}:
            return False
        _require_device(audio)
        side = _side_stream(audio.device)
        side.wait_stream(torch.cuda.current_stream(audio.device))
        # the side stream reads `audio`: keep its block from being recycled to the main stream while it does
        audio.record_stream(side)
        with torch.cuda.stream(side):
            # stage 2: only the frozen prefix (conv stack + layers below the unfrozen ones) runs ahead; the
            # trainable layers run in the step itself, after the optimizer has updated them.  late / concat /
            # gated: the fp32 hidden states their encode() / forward() pool (the pooling and classifier train)
            if stage2:
                kind, out = "prefix", self.audio_model.encode_prefix(audio)
            elif xattn:  # consumed by the next step's head forward, before the encoder graph's next replay
                with G.borrow_outputs():
                    kind, out = "seq", self.audio_model.encode_sequence(audio)
            else:
                kind, out = "hidden", self.audio_model.encode_sequence(audio, out_dtype=torch.float32)
        # the tensor itself (not its address) identifies the batch: a recycled address cannot match
        self._prefetched = (audio, audio._version, out, side, kind)
        return True

    def queue_next_audio(self, audio: torch.Tensor) -> None:
        """Early prefetch: the next xattn ``forward`` starts the audio encoder on ``audio`` (the NEXT batch) on the
        side stream as soon as it has taken its own batch's encoder output -- before the frame trunk -- so the
        encoder overlaps the whole step (forward and backward) instead of the backward only.  A forward that
        cannot use it leaves it queued: ``take_queued_audio`` hands it back (TrainStep then prefetches the old
        way, before the backward)."""
        self._queued_audio = audio

    def take_queued_audio(self):
        a, self._queued_audio = self._queued_audio, None
        return a

    def _issue_queued(self, kind: str, a_out: torch.Tensor, head_seed: bool = True) -> torch.Tensor:
        """Start the queued early prefetch now; returns ``a_out`` made safe against it (a borrowed encoder-graph
        output is rewritten by that replay: this step keeps its own copy, ordered before the side stream).
        ``head_seed``: draw this step's head dropout seed first (the modes with a fusion head)."""
        nxt = self._queued_audio
        if nxt is None or not torch.is_grad_enabled():
            return a_out
        self._queued_audio = None
        if G.is_borrowed(a_out):
            a_out = a_out.clone()
        # host draws in the inline order: this step's head seed before the next batch's encoder draws
        if self.training and head_seed:
            self._head_seed = _next_seed()
        if not self.prefetch_audio(nxt):
            self._queued_audio = nxt
        return a_out

    def _prefetch_matches(self, audio: torch.Tensor, kind: str) -> bool:
        pf = self._prefetched
        return pf is not None and pf[0] is audio and pf[1] == audio._version and pf[4] == kind

    def _take_prefetched(self, audio: torch.Tensor, kind: str):
        """The prefetched result of ``kind`` for exactly this waveform tensor (now ordered after the side stream
        on the current stream), or None."""
        ok = self._prefetch_matches(audio, kind)
        pf, self._prefetched = self._prefetched, None
        if not ok:
            return None
        pf = (None, pf[2], pf[3], pf[4])
        cur = torch.cuda.current_stream(audio.device)
        cur.wait_stream(pf[2])
        for tsr in (pf[1] if isinstance(pf[1], tuple) else (pf[1],)):
            if isinstance(tsr, torch.Tensor):
                tsr.record_stream(cur)
        return pf[1]

    # ---- data-parallel support (dist.GradAllReduce) ----
    def unused_parameters(self):
        """Trainable parameters the configured mode never reaches in forward, so they never get a gradient
        (torch's Adam skips them forever): kept out of the optimizer's flat buffers and the all-reduce."""
        dead = []
        xattn = self.mode in {"xattn", "xattn_concat", "xattn_gated"}
        if xattn:
            dead += list(self.audio_time_conv.parameters())  # fusion.py:273, mel fallback only
        if self.mode != "late":
            # the encoders' own classifier heads are only used by late fusion (and audio/video-only models)
            for enc in (self.audio_model, self.video_model):
                cls = getattr(enc, "classifier", None)
                if cls is None:
                    continue
                if enc is self.audio_model and not xattn and getattr(enc, "embedding_dim", 768) != enc.sequence_dim:
                    dead += list(cls[3].parameters())  # encode() uses classifier[0] when the dims differ
                else:
                    dead += list(cls.parameters())
            if xattn:  # the backbone / encode_sequence are called directly: the encoders' poolers are unused
                for enc in (self.audio_model, self.video_model):
                    tp = getattr(enc, "temporal_pool", None)
                    if tp is not None:
                        dead += list(tp.parameters())
        return dead

    def may_skip_grads(self) -> bool:
        """True when some step can leave a used trainable parameter without a gradient (gated ModalityDropout;
        WavLM LayerDrop over trainable encoder layers): the data-parallel "has a gradient" set is then synced."""
        wav = getattr(self.audio_model, "wavlm", None)
        return self.mode == "gated" or (wav is not None and wav.trainable())

    def early_grad_params(self):
        """The parameters whose gradients are final once the ResNet18 backward has enqueued blocks >=
        ``video.SPLIT_BLOCK``: the fusion head, the video encoder's head and those trunk blocks (a STATIC list:
        dist.GradAllReduce fixes its early-bucket boundaries from it, identically on every rank)."""
        from .video import SPLIT_BLOCK

        trunk = self.video_model.backbone
        if not hasattr(trunk, "split_params"):
            return []
        head = [q for n, q in self.named_parameters() if not n.startswith(("audio_model.", "video_model."))]
        vid_head = [q for n, q in self.video_model.named_parameters() if not n.startswith("backbone.")]
        return head + vid_head + list(trunk.split_params(SPLIT_BLOCK))

    def register_grad_ready_hook(self, fn) -> None:
        """``fn(params)`` is called from the backward as soon as the ``early_grad_params()`` gradients are final
        (enqueued): the early all-reduce bucket (dist.GradAllReduce)."""
        trunk = self.video_model.backbone
        early = self.early_grad_params()
        trunk.grad_ready_hook = lambda ps: fn(early)

    def pop_alignment_loss(self) -> Optional[torch.Tensor]:
        loss = self.alignment_loss
        self.alignment_loss = None
        return loss

    # -------------------------------------------------------------------------------------
    def head_config(self) -> XH.HeadConfig:
        return XH.HeadConfig(num_heads=self.num_heads, xattn_head=self.xattn_head,
                             use_prior=self.emotion_prior_bias is not None, attn_dropout=self.attn_dropout,
                             drop_path=self.v_drop_path.drop_prob, mlp_dropout=self._mlp_dropout_p(),
                             prior_dropout=(self.emotion_prior_bias.dropout if self.emotion_prior_bias is not None else 0.0),
                             temporal_pooling=self.temporal_pooling, temporal_num_heads=self.temporal_num_heads,
                             temporal_num_layers=self.temporal_num_layers, temporal_dropout=self.temporal_dropout)

    def _mlp_dropout_p(self) -> float:
        seq = self.xattn_mlp if self.xattn_head == "concat" else self.xattn_gate
        return float(seq[2].p)  # the nn.Dropout(0.2) of fusion.py:312-324

    def head_params(self):
        """(names, params) of the fusion head (everything outside the two encoders), listed once."""
        hp = self.__dict__.get("_mer_head_params")
        if hp is None:
            names, params = [], []
            for n, q in self.named_parameters():
                if n.startswith(("audio_model.", "video_model.")):
                    continue
                names.append(n)
                params.append(q)
            hp = self.__dict__["_mer_head_params"] = (tuple(names), params)
        return hp

    def xattn_from_features(self, v_feat: torch.Tensor, a_seq: torch.Tensor) -> torch.Tensor:
        """xattn head on encoder features: v_feat [B,T,v_dim] (backbone output), a_seq [B,Ta,seq_dim]."""
        _require_device(v_feat, a_seq)
        names, params = self.head_params()
        qlin = EH.int8_images(self)
        if qlin is not None:  # INT8 inference (TorchModelRunner enable_dynamic_quant): forward only
            with torch.no_grad():
                return XH.head_forward(dict(zip(names, params)), self.head_config(), v_feat.contiguous(),
                                       a_seq.contiguous(), False, None, qlin=qlin)[0]
        cfg = self.head_config()
        v_feat, a_seq = v_feat.contiguous(), a_seq.contiguous()
        runner = self._head_runner(names, params, cfg, v_feat, a_seq)
        if runner is None:  # the eager head keeps its inputs for the backward: own copies of borrowed outputs
            v_feat = v_feat.clone() if G.is_borrowed(v_feat) else v_feat
            a_seq = a_seq.clone() if G.is_borrowed(a_seq) else a_seq
        rng = self.step_rng(v_feat.device) if (self.training and runner is None) else None
        return _XattnHeadFn.apply(v_feat, a_seq, cfg, self.training, rng, names, runner, *params)

    def _head_runner(self, names, params, cfg, v_feat, a_seq):
        """The captured-graph runner of the head for these shapes, or None (eager) while warming up, during
        a capture, for a second forward before the first one's backward, or with input gradients wanted
        for the audio features (graphs.py)."""
        if G.capturing() or a_seq.requires_grad:
            return None
        key = (tuple(v_feat.shape), tuple(a_seq.shape), a_seq.dtype, v_feat.device.index, self.training,
               dataclasses.astuple(cfg), tuple(q.data_ptr() for q in params))
        if not self._head_graphs.ready(key):
            return None
        r = self._head_graphs.get(key)
        if r is None:
            r = self._head_graphs.put(key, _HeadGraphs(self, names, cfg, self.training))
        if r.pending:
            return None
        r.cur_gen = r.claim(torch.is_grad_enabled())
        return r

    def forward(self, video: torch.Tensor, audio: torch.Tensor):
        self.alignment_loss = None
        _require_device(video, audio)
        if self.mode == "late":
            hidden = self._take_prefetched(audio, "hidden")
            drop_seed = None
            if hidden is not None and self._queued_audio is not None and torch.is_grad_enabled():
                # early prefetch (as in the other modes): the next batch's encoder starts now and overlaps this whole
                # step instead of the backward only (late ran 181 steps/s against 208 for concat without it).  This
                # step's own host draw -- the audio classifier's dropout seed -- comes first, as in the inline
                # schedule, whose next-batch encoder draws all happen after it; late mode has no head seed
                drop_seed = self.audio_model.draw_dropout_seed()
                hidden = self._issue_queued("hidden", hidden, head_seed=False)
            a_logits = self.audio_model(audio) if hidden is None else self.audio_model(audio, hidden=hidden,
                                                                                         drop_seed=drop_seed)
            v_logits = self.video_model(video)
            return self._late_tail(a_logits, v_logits)

        if self.mode in {"xattn", "xattn_concat", "xattn_gated"}:
            b, t, c, h, w = video.shape
            v_in = video.view(b * t, c, h, w)
            if not hasattr(self.audio_model, "encode_sequence"):
                raise NotImplementedError("the audio_time_conv fallback (fusion.py:379-384) for an audio model without "
                                          "encode_sequence is not built: WavLMAudioEncoder and AudioNet both have it")
            # The two encoders are independent until the xattn block (fusion.py:369-378): the (frozen,
            # forward-only) audio encoder runs on a side HIP stream concurrently with the frame trunk, so
            # its GEMMs fill the CUs the trunk's smaller convs and BatchNorm passes leave idle.  When
            # prefetch_audio() already started it for this very batch (during the previous step's
            # backward), its result is taken over instead.
            # an audio model without a WavLM encoder (the mel AudioNet) is never prefetched: it takes the inline path
            kind = "seq" if self.audio_encoder_frozen() else "prefix"
            if self._prefetch_matches(audio, kind):
                got = self._issue_queued(kind, self._take_prefetched(audio, kind))
                with G.borrow_outputs():
                    v_feat = self.video_model.backbone(v_in).view(b, t, self.v_dim)
                # stage 2: prefetched frozen prefix -> trainable tail now
                a_seq = self.audio_model.encode_sequence(audio, prefix=got) if kind == "prefix" else got
                return self.xattn_from_features(v_feat, a_seq)
            self._prefetched = None
            side = _side_stream(video.device)
            # the encoders' graph outputs go to the head without a copy (graphs.borrow_outputs; the head's
            # graph copies them into its static inputs, an eager head takes its own copy)
            with G.borrow_outputs():
                if side is not None:
                    cur = torch.cuda.current_stream(video.device)
                    side.wait_stream(cur)
                    with torch.cuda.stream(side):
                        a_seq = self.audio_model.encode_sequence(audio)
                    v_feat = self.video_model.backbone(v_in).view(b, t, self.v_dim)
                    cur.wait_stream(side)
                    a_seq.record_stream(cur)
                else:
                    a_seq = self.audio_model.encode_sequence(audio)
                    v_feat = self.video_model.backbone(v_in).view(b, t, self.v_dim)
            if kind == "seq":  # (the first step of an early-prefetch run: nothing was prefetched for it yet)
                a_seq = self._issue_queued(kind, a_seq)
            return self.xattn_from_features(v_feat, a_seq)

        if self.mode not in {"concat", "gated"}:
            raise ValueError(f"Unknown fusion mode: {self.mode}")
        hidden = self._take_prefetched(audio, "hidden")
        # gated: ModalityDropout (fusion.py:430) replaces a projection by zeros_like -- the dropped branch and
        # everything feeding only it get NO gradient (torch's Adam then skips them), see embedding_head
        gated = self.mode == "gated"
        drops = None
        if hidden is not None:
            # early prefetch: the next batch's encoder starts now and overlaps this whole step (as in xattn mode).
            # This step's own host draws (modality dropout here, the head's seed in _issue_queued) come first, as
            # in the inline schedule, whose encoder draws all happen after them
            drops = self.modality_dropout.draw() if gated else (False, False)
            hidden = self._issue_queued("hidden", hidden)
        a_emb = self.audio_model.encode(audio) if hidden is None else self.audio_model.encode(audio, hidden=hidden)
        v_emb = self.video_model.encode(video)
        return self._embedding_tail(a_emb, v_emb, drops)

    def _embedding_tail(self, a_emb: torch.Tensor, v_emb: torch.Tensor, drops=None) -> torch.Tensor:
        """concat / gated from the two encoders' embeddings on: the optional alignment, this step's modality-dropout
        draw (unless ``drops`` was drawn ahead of an early prefetch) and the head."""
        if self.semantic_alignment is not None:  # fusion.py:417-418
            a_emb, v_emb, self.alignment_loss = self.semantic_alignment(a_emb, v_emb)
        if drops is None:
            drops = self.modality_dropout.draw() if self.mode == "gated" else (False, False)
        return EH.embedding_head(self, a_emb, v_emb, *drops)

    @staticmethod
    def _late_tail(a_logits: torch.Tensor, v_logits: torch.Tensor) -> torch.Tensor:
        """late from the two encoders' logits on (fusion.py:358-363)."""
        return EH.late_probs(a_logits, v_logits)

    def forward_from_frame_features(self, v_feat: torch.Tensor, audio: torch.Tensor) -> torch.Tensor:
        """``forward`` from the frame trunk's output on: ``v_feat`` ``[B, T, 512]`` fp32 (``video_model.backbone`` per
        frame), ``audio`` as ``forward`` takes it.  In eval mode the trunk is a per-frame function (BatchNorm on
        running statistics), so a caller whose clips share frames -- the overlapping windows of a recording,
        ``TorchModelRunner.predict_timeline`` -- encodes each frame once and gathers the rows.  Eval only; the audio
        encoder runs inline on the current stream."""
        if self.training:
            raise RuntimeError("forward_from_frame_features is an eval-mode entry point (in training mode BatchNorm "
                               "makes the trunk a function of the whole batch): call .eval()")
        _require_device(v_feat, audio)
        if v_feat.dim() != 3:
            raise ValueError(f"v_feat must be trunk features [B, T, dim], got {tuple(v_feat.shape)}")
        self.alignment_loss = None
        if self.mode in {"xattn", "xattn_concat", "xattn_gated"}:
            return self.xattn_from_features(v_feat, self.audio_model.encode_sequence(audio))
        if self.mode not in {"late", "concat", "gated"}:
            raise ValueError(f"Unknown fusion mode: {self.mode}")
        if self.mode == "late":
            return self._late_tail(self.audio_model(audio), self.video_model.forward_from_frame_features(v_feat))
        return self._embedding_tail(self.audio_model.encode(audio), self.video_model.temporal_pool(v_feat))
