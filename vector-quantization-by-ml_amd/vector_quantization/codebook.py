"""``Codebook``: the stateful holder of the code vectors, re-written around ONE native search op.

Mirrors the constructor signature, buffer names (= checkpoint format: ``embeddings``, ``embed_avg``,
``cluster_size``) and return convention of the reference class
(/root/reference/vector_quantization/codebooks.py:81-435), but never materialises the ``[h, M, K]``
similarity / one-hot tensors the reference builds on every call (codebooks.py:386-390,
utils/general.py:129): search + gather (+ straight-through + squared error) is a single HIP launch.

What is native here: the forward search/gather (``search.quantize_rows``).  What is plain PyTorch on
the same device (training-state bookkeeping that comes AFTER the hot path): EMA statistics,
dead-code re-seeding, k-means seeding (which reuses the native search for its assignment step).
"""
from __future__ import annotations

from dataclasses import asdict, is_dataclass

import torch
import torch.distributed as dist
import torch.nn.functional as F
from torch import nn

from . import search
from .params import GumbelParams, KmeansParameters


def _identity(t):
    return t


def _unit_rows(t):
    return F.normalize(t, p=2, dim=-1)


_ROW_TRANSFORMS = {"identity": _identity, "l2norm": _unit_rows}


def _row_transform(name: str, what: str):
    if name not in _ROW_TRANSFORMS:
        # the reference does `raise "<str>"`, which surfaces as a TypeError (codebooks.py:110,117)
        raise TypeError(f"The option {name} for {what} is not implemented")
    return _ROW_TRANSFORMS[name]


def _default_codebook(h: int, k: int, d: int) -> torch.Tensor:
    """Same distribution as the reference's default (kaiming_uniform_ on [h, K, D]: fan_in = K * D)."""
    t = torch.empty(h, k, d)
    nn.init.kaiming_uniform_(t)
    return t


def _pick_rows(rows: torch.Tensor, count: int) -> torch.Tensor:
    """`count` rows of a [N, D] tensor: a random subset when N >= count, else draws with replacement."""
    n = rows.shape[0]
    if n >= count:
        sel = torch.randperm(n, device=rows.device)[:count]
    else:
        sel = torch.randint(0, n, (count,), device=rows.device)
    return rows[sel]


def _pick_rows_all_ranks(rows: torch.Tensor, count: int) -> torch.Tensor:
    """`count` rows drawn from the union of every rank's rows, IDENTICAL on all ranks (utils/distributed.py:56-78): rank 0
    splits `count` over the ranks in proportion to their row counts (sequential binomial draws), every rank samples its share
    locally, the shares are exchanged.  Replicas that seed or re-seed codes from this keep bit-identical codebooks."""
    world, rank = dist.get_world_size(), dist.get_rank()
    sizes = [torch.zeros((), dtype=torch.long, device=rows.device) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor(rows.shape[0], dtype=torch.long, device=rows.device))
    sizes = torch.stack(sizes)
    if rank == 0:
        probs = (sizes / sizes.sum()).cpu()
        left = probs.new_full((), count)
        remainder = probs.new_ones(())
        share = torch.empty_like(probs, dtype=torch.long)
        for i, p in enumerate(probs):
            drawn = torch.binomial(left, p / remainder)
            share[i] = drawn
            left -= drawn
            remainder -= p
        assert left == 0, f"invalid total count {left}"
        share = share.to(rows.device)
    else:
        share = torch.empty_like(sizes)
    dist.broadcast(share, src=0)
    share = share.tolist()
    mine = _pick_rows(rows, share[rank])
    parts = []
    for src, n in enumerate(share):
        part = mine if src == rank else rows.new_empty((n, *rows.shape[1:]))
        if n > 0:  # (every rank knows the shares: empty ones are skipped consistently)
            dist.broadcast(part, src=src)
        parts.append(part)
    return torch.cat(parts, dim=0)


def _affine_std(variance: torch.Tensor) -> torch.Tensor:
    return variance.clamp(min=1e-5).sqrt()


def set_expire_on_device(module: nn.Module, enabled: bool = True) -> nn.Module:
    """Switch every ``Codebook`` below ``module`` to (or back from) dead-code expiry on the device: the training forward then
    never waits for the GPU and can be captured in a graph (graphs.GraphedTrainForward).  The replacement rows are then chosen
    by the rule of vq_expire_codes_f32 from ONE seed drawn from torch's generator per expiry step, not by randperm / randint."""
    for m in module.modules():
        if isinstance(m, Codebook):
            m.expire_on_device = bool(enabled)
    return module


class _AffineCodes(torch.autograd.Function):
    """codes [h, K, D] -> (codes - codebook_mean) * (batch_std / codebook_std) + batch_mean, natively (vq_affine_apply_f32,
    mode 0) when ``fused`` is the backend's hook, else with the reference's own op sequence.  Backward: g * scale; the scale
    is made (and kept: the statistics move in place with the next forward) only when the codes ask for a gradient."""

    @staticmethod
    def forward(ctx, codes, fused, codebook_mean, codebook_variance, batch_mean, batch_variance):
        scale = None
        if ctx.needs_input_grad[0] or fused is None:
            scale = _affine_std(batch_variance) / _affine_std(codebook_variance)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(scale)
        if fused is not None:
            return fused(codes.detach().contiguous(), codebook_mean, codebook_variance, batch_mean, batch_variance, mode=0)
        return (codes - codebook_mean) * scale + batch_mean

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None, None, None, None


class Codebook(nn.Module):
    def __init__(
        self,
        dim,
        codebook_size,
        num_codebooks=1,
        initialization_by_kmeans: bool = False,
        kmeans_params: KmeansParameters = None,
        decay: float = 0.8,
        eps_for_smoothing: float = 1e-5,
        threshold_ema_dead_code: int = 2,
        reset_cluster_size: int = None,
        use_ddp: bool = False,
        distributed_replace_codes: bool = True,
        learnable_codebook: bool = False,
        gumbel_params: GumbelParams = None,
        ema_update: bool = True,
        use_affine: bool = False,
        affine_params=None,
        transform_input: str = "identity",
        use_cosine_sim: bool = False,
        weights_regularization: str = "identity",
    ):
        super().__init__()
        self.transform_input = _row_transform(transform_input, "transform input function")
        self.weights_regularization = _row_transform(weights_regularization, "weights regularization")
        if use_affine and affine_params is None:
            # (the reference accepts this and fails with AttributeError on its first forward, codebooks.py:288)
            raise ValueError("use_affine=True needs affine_params (AffineParameters, or the dict dataclasses.asdict makes of it)")

        self.dim = dim
        self.codebook_size = codebook_size
        self.num_codebooks = num_codebooks
        self.use_cosine_sim = use_cosine_sim
        self.metric = search.DOT if use_cosine_sim else search.EUCLID
        self.decay = decay
        self.ema_update = ema_update
        self.eps_for_smoothing = eps_for_smoothing
        self.threshold_ema_dead_code = threshold_ema_dead_code
        self.reset_cluster_size = threshold_ema_dead_code if reset_cluster_size is None else reset_cluster_size
        self.use_ddp = use_ddp
        self.distributed_replace_codes = distributed_replace_codes
        self.learnable_codebook = learnable_codebook
        self.use_affine = bool(use_affine)
        self.affine_params = None
        if use_affine:
            self.affine_params = asdict(affine_params) if is_dataclass(affine_params) else dict(affine_params)

        if kmeans_params is None:
            kmeans_params = KmeansParameters() if initialization_by_kmeans else None
        self.kmeans_params = asdict(kmeans_params) if is_dataclass(kmeans_params) else kmeans_params
        if gumbel_params is None:
            gumbel_params = GumbelParams()
        self.gumbel_params = asdict(gumbel_params) if is_dataclass(gumbel_params) else dict(gumbel_params)
        assert not (self.gumbel_params.get("reinmax", False) and not self.gumbel_params.get("straight_through", False)), (
            "reinmax can only be turned on if using straight through gumbel softmax"
        )

        assert not (use_ddp and num_codebooks > 1 and initialization_by_kmeans), (
            "kmeans init is not compatible with multiple codebooks in distributed environment for now"
        )

        start = torch.zeros(num_codebooks, codebook_size, dim) if initialization_by_kmeans else _default_codebook(
            num_codebooks, codebook_size, dim)
        start = self.weights_regularization(start)
        self.is_initialized = not initialization_by_kmeans
        self.register_buffer("cluster_size", torch.zeros(num_codebooks, codebook_size))
        self.register_buffer("embed_avg", start.clone())
        if learnable_codebook:
            self.embeddings = nn.Parameter(start)
        else:
            self.register_buffer("embeddings", start)
        if use_affine:
            if self.gumbel_params.get("straight_through", False):
                raise NotImplementedError("use_affine together with GumbelParams(straight_through=True) is not supported: "
                                          "the relaxation's gradient is provided for untransformed codes only")
            # codebooks.py:192-206: names, shapes and dtypes are the checkpoint format.  The two batch buffers stay None until
            # the first forward; afterwards every statistic is updated IN PLACE (the reference re-registers new tensors)
            self.register_buffer("batch_mean", None)
            self.register_buffer("batch_variance", None)
            self.register_buffer("codebook_mean_needs_init", torch.Tensor([True]))
            self.register_buffer("codebook_mean", torch.zeros(num_codebooks, 1, dim))
            self.register_buffer("codebook_variance_needs_init", torch.Tensor([True]))
            self.register_buffer("codebook_variance", torch.zeros(num_codebooks, 1, dim))
        # opt-in (set_expire_on_device): dead codes are found and re-seeded by launches that never make the host wait, with
        # rows chosen by a counter-based rule instead of torch.randperm / randint.  Not part of the state_dict.
        self.expire_on_device = False
        # host-side mirror of the two *_needs_init flags (no device read in steady state; refreshed by load_state_dict)
        self._codebook_stats_need_init = True
        # the statistics the current forward uses (update_affine) and the effective codes made from them
        self._affine_now = None
        self._effective = None
        # packed image of `embeddings` for the native search, rebuilt only when the codes change (see packed_codes)
        self._packed = None
        self._packed_key = None
        self._packed_epoch = 0
        # screen image of `_packed` for the screened sweep, one per stream that runs this module (see screen_codes)
        self._screen = {}
        self._screen_key = None

    # ------------------------------------------------------------------ helpers
    def _stochastic_requested(self) -> bool:
        """The reference always samples through ``sample_fn_training`` (codebooks.py:388), whose ``training`` flag is
        GumbelParams.training (default True) -- NOT the module's train / eval state."""
        g = self.gumbel_params
        return bool(g.get("training", True) and g.get("stochastic", False) and g.get("temperature", 1.0) > 0)

    def _relaxation_active(self) -> bool:
        """The selection is differentiated through softmax(similarities / temperature) (utils/general.py:135): asked for,
        at a positive temperature, with GumbelParams.training, and -- the reference gathers by index in eval mode
        (codebooks.py:393-397) -- only while the module trains."""
        g = self.gumbel_params
        return bool(self.training and g.get("straight_through", False) and g.get("training", True)
                    and g.get("temperature", 1.0) > 0)

    def _sync_sum(self, t: torch.Tensor) -> torch.Tensor:
        if self.use_ddp and dist.is_available() and dist.is_initialized():
            dist.all_reduce(t)
        return t

    def current_codes(self) -> torch.Tensor:
        return self.embeddings if self.learnable_codebook else self.embeddings.detach()

    def codes_state(self):
        """Identity of the code values: storage, in-place version counter (``copy_`` / ``load_state_dict`` / optimizer steps
        bump it) and an epoch for writes the counter cannot see (``.data`` index writes, the native EMA kernel)."""
        e = self.embeddings
        if e.is_inference():  # built / loaded under torch.inference_mode(): no version counter -> never reuse a packed image
            return (e.data_ptr(), object(), self._packed_epoch, e.device, tuple(e.shape))
        return (e.data_ptr(), e._version, self._packed_epoch, e.device, tuple(e.shape))

    def invalidate_packed(self):
        """Call after changing ``embeddings`` through ``.data`` or a raw pointer (every writer in this package does)."""
        self._packed_epoch += 1
        self._effective = None
        self._screen = {}
        self._screen_key = None

    def packed_codes(self):
        """Packed image [h, packed_floats] of the codes for the native search (None for backends without one), cached:
        an inference forward does not re-pack an unchanged codebook (13 us at K=1024 D=256, 121 us at K=65536 D=512)."""
        backend = search.get_backend()
        if not getattr(backend, "uses_packed", False):
            return None
        if self.use_affine:
            # the effective codes change with every forward's statistics: an image is packed per call, never cached
            codes = self.effective_codes().detach()
            if not codes.is_cuda and not torch.compiler.is_compiling():
                return None
            with torch.no_grad():
                return backend.pack(codes.contiguous(), self.metric)
        if torch.compiler.is_compiling():  # traced: the pack is a node of the graph (no identity-keyed cache inside a trace)
            return backend.pack(self.embeddings.detach().contiguous(), self.metric)
        if not self.embeddings.is_cuda:
            return None
        key = (self.codes_state(), self.metric)
        if self._packed_key != key:
            with torch.no_grad():
                self._packed = backend.pack(self.embeddings.detach().contiguous(), self.metric)
            self._packed_key = key
        return self._packed

    _SCREEN_STREAMS = 4  # images kept: one per stream that ran this module last

    def screen_codes(self):
        """The screen image of ``packed_codes()`` for inference searches (``backend.pack_screen``), cached like the packed
        image: an inference forward of an unchanged codebook launches no pack kernel at all.  The image ends in the counts
        that the kernels of one call share, so two streams that run this module at the same time must not share one: the
        current stream is part of the key, and the few most recent streams keep theirs.  None: backends without one, affine
        codebooks (their codes change with every forward), traced or graph-captured forwards (the pack stays a node of the
        graph, which reads the weights of its own time) and shapes the screened sweep does not take."""
        backend = search.get_backend()
        if (not getattr(backend, "uses_packed", False) or not hasattr(backend, "pack_screen") or self.use_affine
                or torch.compiler.is_compiling() or not self.embeddings.is_cuda or self.metric != search.EUCLID
                or torch.cuda.is_current_stream_capturing()):
            return None
        packed = self.packed_codes()
        key = self._packed_key
        if self._screen_key != key:
            self._screen, self._screen_key = {}, key
        stream = torch.cuda.current_stream(self.embeddings.device).cuda_stream
        if stream not in self._screen:
            h, k, d = self.embeddings.shape
            while len(self._screen) >= self._SCREEN_STREAMS:
                self._screen.pop(next(iter(self._screen)))
            with torch.no_grad():
                self._screen[stream] = backend.pack_screen(packed, h, k, d, self.metric)
        return self._screen[stream]

    # ------------------------------------------------------------------ affine re-parameterisation
    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        if self.use_affine:
            for name in ("batch_mean", "batch_variance"):  # absent (None) until the first forward: make room for saved ones
                saved = state_dict.get(prefix + name)
                if saved is not None and getattr(self, name) is None:
                    setattr(self, name, torch.empty_like(saved, device=self.embeddings.device))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if self.use_affine:
            self._codebook_stats_need_init = bool(self.codebook_mean_needs_init.item() != 0
                                                  or self.codebook_variance_needs_init.item() != 0)
            self._affine_now = None
            self._effective = None

    @staticmethod
    def _fused_affine(name: str):
        """The backend's native affine hook (``column_stats`` / ``affine_apply``), or None: backends without it, traced
        forwards (torch.compile runs the step as tensor ops) and VQ_NO_FUSED_AFFINE=1 in the environment (A/B measurements;
        read per call: tests compare both paths in one process) take the tensor-op path."""
        import os

        if torch.compiler.is_compiling() or os.environ.get("VQ_NO_FUSED_AFFINE"):
            return None
        return getattr(search.get_backend(), name, None)

    def _moments(self, rows: torch.Tensor, flat_mask=None):
        """rows [h, M, D] -> (count [h] (int64 from the kernel), mean [h, 1, D], m2 [h, 1, D]) over the kept rows."""
        fused = self._fused_affine("column_stats")
        if fused is not None:
            count, mean, m2 = fused(rows, flat_mask)
            return count, mean[:, None], m2[:, None]
        if flat_mask is not None:
            rows = rows[flat_mask].reshape(rows.shape[0], -1, rows.shape[-1])  # (the same rows are kept in every head)
        mean = rows.mean(dim=1, keepdim=True)
        m2 = torch.var(rows, dim=1, unbiased=False, keepdim=True) * rows.shape[1]
        return torch.full((rows.shape[0],), float(rows.shape[1]), device=rows.device), mean, m2

    def _mean_and_variance(self, rows: torch.Tensor, flat_mask=None, sync: bool = False):
        """Per-column mean and biased variance [h, 1, D] of the kept rows (codebooks.py:287-292, 309-314); with ``sync`` over
        the rows of every rank (codebooks.py:319-348) from each rank's (n, mean, M2) alone.  A head whose mask keeps no row
        gets NaN statistics (0 / 0), as the reference's mean over no rows does."""
        if not sync and self._fused_affine("column_stats") is None:  # the reference's own two reductions
            if flat_mask is not None:
                rows = rows[flat_mask].reshape(rows.shape[0], -1, rows.shape[-1])
            return rows.mean(dim=1, keepdim=True), torch.var(rows, dim=1, unbiased=False, keepdim=True)
        count, mean, m2 = self._moments(rows, flat_mask)
        n = count[:, None, None]
        if not sync:
            return mean, m2 / n
        n = n.to(mean.dtype)
        total = n.clone()
        dist.all_reduce(total)
        column_sum = mean * n
        dist.all_reduce(column_sum)
        global_mean = column_sum / total
        # sum of squared deviations about the GLOBAL mean from the local ones: no second pass over the rows
        about_global = m2 + n * (mean - global_mean) ** 2
        dist.all_reduce(about_global)
        return global_mean, about_global / total

    @staticmethod
    def _decay_into(buffers, fresh, decay: float):
        """buffers <- buffers * decay + fresh * (1 - decay), in place, two launches for the pair (codebooks.py:271)."""
        torch._foreach_mul_(buffers, decay)
        torch._foreach_add_(buffers, fresh, alpha=1 - decay)

    @torch.no_grad()
    def update_affine(self, flat: torch.Tensor, flat_mask=None):
        """codebooks.py:275-348, at the top of every search (train AND eval): running column statistics of the codes (moved
        only while training) and of the batch (always), updated in place.  flat [h, M, D] (strided views are not copied)."""
        assert self.use_affine
        p = self.affine_params
        flat = flat.detach()
        if flat.dtype != torch.float32:
            flat = flat.float()
        self._effective = None
        codebook_mean, codebook_variance = self.codebook_mean, self.codebook_variance
        if self.training or self._codebook_stats_need_init:
            mean, var = self._mean_and_variance(self.embeddings.detach())
            if not self.training:
                # eval before any training forward: the reference searches against torch.empty garbage; here the statistics
                # of the current codes serve this forward and are not stored
                codebook_mean, codebook_variance = mean, var
            elif self._codebook_stats_need_init:
                self.codebook_mean.copy_(mean)
                self.codebook_variance.copy_(var)
                self.codebook_mean_needs_init.zero_()
                self.codebook_variance_needs_init.zero_()
                self._codebook_stats_need_init = False
            else:
                self._decay_into([self.codebook_mean, self.codebook_variance], [mean, var], p["codebook_decay"])
        sync = bool(p["sync"]) and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        mean, var = self._mean_and_variance(flat, flat_mask, sync=sync)
        if self.batch_mean is None:
            self.batch_mean, self.batch_variance = mean.clone(), var.clone()
        else:
            self._decay_into([self.batch_mean, self.batch_variance], [mean, var], p["batch_decay"])
        self._affine_now = (codebook_mean, codebook_variance, self.batch_mean, self.batch_variance)

    def effective_codes(self) -> torch.Tensor:
        """The codes the forward consumes: ``current_codes()``, under affine moved to the batch's moments (codebooks.py:379-384):
        (embeddings - codebook_mean) * (batch_std / codebook_std) + batch_mean.  Differentiable with respect to a learnable
        codebook (the statistics are constants).  Without a gradient they are made once per forward (update_affine drops the
        previous ones); a tensor that carries an autograd graph is never kept on the module (it would keep the graph alive
        between steps and make the module impossible to deep-copy): a learnable codebook makes them per consumer."""
        codes = self.current_codes()
        if not self.use_affine:
            return codes
        if self._affine_now is None:
            raise RuntimeError("an affine codebook has no statistics yet: update_affine() runs at the top of every forward")
        if codes.requires_grad and torch.is_grad_enabled():
            return _AffineCodes.apply(codes, self._fused_affine("affine_apply"), *self._affine_now)
        key = self.codes_state()
        if self._effective is None or self._effective[0] != key:
            with torch.no_grad():
                made = _AffineCodes.apply(codes.detach(), self._fused_affine("affine_apply"), *self._affine_now)
            self._effective = (key, made)
        return self._effective[1]

    # ------------------------------------------------------------------ the hot path
    def quantize_flat(self, flat: torch.Tensor, *, ste: bool = False, want_sq_err: bool = False,
                      codebook_grad_from_err: bool = False, out=None, idx=None, want_lse: bool = False,
                      frozen: bool = False, rotate: bool = False):
        """flat [h, M, D] (strided rows fine) -> (out [h, M, D], idx [h, M] int64, sq_err [1] float64 | None).
        ``rotate``: with ``ste``, the rows receive the rotation trick's gradient of the output instead of the
        straight-through one (search.quantize_rows); nothing that is returned changes.
        ``want_lse``: a fourth element (lse [h, M], target_logit [h, M]) -- log-sum-exp of the row's similarities and the
        similarity of the chosen code, from the same sweep -- or None when the sampling is stochastic.
        ``frozen``: the caller will NOT run the EMA update after this search (freeze_codebook)."""
        if self._stochastic_requested():
            res = self._quantize_stochastic(flat, ste=ste, want_sq_err=want_sq_err,
                                            codebook_grad_from_err=codebook_grad_from_err, idx=idx, rotate=rotate)
            return (*res, None) if want_lse else res
        codes = self.effective_codes()
        packed = self.packed_codes()
        if (self._relaxation_active() and torch.is_grad_enabled() and (flat.requires_grad or codes.requires_grad)
                and (not ste or (want_sq_err and codebook_grad_from_err))):
            # (with the straight-through output and a detached squared error nothing consumes the relaxation's gradient:
            # the single launch below stays -- VectorQuantize with an EMA codebook, where the reference discards it too)
            res = self._quantize_relaxed(flat, codes, packed, ste=ste, want_sq_err=want_sq_err,
                                         codebook_grad_from_err=codebook_grad_from_err, idx=idx, frozen=frozen)
            return (*res, None) if want_lse else res
        if (torch.is_grad_enabled() and flat.requires_grad and not codes.requires_grad and self.training and self.ema_update
                and not frozen and not self.use_affine):  # (effective codes are a tensor of this forward already)
            # the EMA step that follows rewrites the codebook in place; the backward pass (commitment loss: 2 (x - c))
            # must see the codes this forward used, as the reference's autograd graph does (it holds `quantize` by value)
            codes = codes.clone()
        # (the search sweep emits the log-sum-exp only for rows one launch holds; wider rows leave it to the loss)
        lse_here = want_lse and flat.shape[-1] <= search.LSE_MAX_DIM
        # (the screened sweep takes plain inference searches only: the others would build the image for nothing)
        screen = self.screen_codes() if not (ste or want_sq_err or want_lse) else None
        try:
            res = search.quantize_rows(flat, codes[:, None], metric=self.metric, ste=ste, want_sq_err=want_sq_err,
                                       codebook_grad_from_err=codebook_grad_from_err, out=out, idx=idx, want_lse=lse_here,
                                       packed=packed, screen=screen, rotate=rotate)
        except Exception:
            self._screen = {}  # a call that failed may have left its counts behind in the image
            raise
        out, idx, sq_err = res[:3]
        if want_lse and not lse_here:
            return out, idx[..., 0], sq_err, None
        if want_lse:
            best = res[3]["best"][..., 0]
            return out, idx[..., 0], sq_err, (res[3]["lse"], best if self.use_cosine_sim else -best)
        return out, idx[..., 0], sq_err

    def _quantize_relaxed(self, flat, codes, packed, *, ste, want_sq_err, codebook_grad_from_err, idx, frozen):
        """Argmax selection with the straight-through / reinmax Gumbel gradient: the search runs as always (indices stay
        bit-exact), the gathered rows go through gumbel.relaxed_gather, the rest is tensor ops on its output."""
        from . import gumbel

        g = self.gumbel_params
        with torch.no_grad():
            try:
                _, ind, _ = search.quantize_rows(flat.detach(), codes.detach()[:, None], metric=self.metric, idx=idx,
                                                 packed=packed, screen=self.screen_codes())
            except Exception:
                self._screen = {}  # a call that failed may have left its counts behind in the image
                raise
        ind = ind[..., 0]
        live = None
        if self.ema_update and not frozen:
            # the EMA step that follows rewrites the codes behind autograd's back: the reference's backward takes the
            # softmax and the distances from the codes of this forward and multiplies with the updated ones
            codes, live = codes.clone(), self.embeddings
        x = flat.float()
        picked = gumbel.relaxed_gather(x, codes, ind, self.metric, g.get("temperature", 1.0), g.get("reinmax", False), live)
        sq_err = None
        if want_sq_err:
            target = picked if codebook_grad_from_err else picked.detach()
            sq_err = ((target - x) ** 2).sum(dtype=torch.float64).reshape(1)
        out = x + (picked - x).detach() if ste else picked
        return out, ind, sq_err

    def _quantize_stochastic(self, flat, *, ste, want_sq_err, codebook_grad_from_err, idx=None, rotate=False):
        """Gumbel-max sampling of the code (utils/general.py:106-129): ind = argmax(similarities / temperature + g),
        g = -log(-log(u)).  RNG-dependent, so no parity with the reference's draws is possible.  Rows of up to 512 dims:
        ONE native sweep (vq_gumbel_sample_f32) that makes the noise in registers from a seed drawn on the device from torch's
        generator -- nothing of [h, M, K] exists.  Wider rows, backends without the sweep and VQ_NO_FUSED_SAMPLE=1 in the
        environment (A/B measurements): similarities from the native kernel in bounded row chunks, noise from torch's generator.
        The straight-through / reinmax relaxations are provided for the argmax selection (_quantize_relaxed), not for
        sampled codes.  ``rotate``: the straight-through output carries the rotation trick's gradient, for the sampled codes."""
        import os

        from . import gumbel as gumbel_mod
        from . import losses

        g = self.gumbel_params
        if g.get("straight_through", False) or g.get("reinmax", False):
            raise NotImplementedError("straight-through / reinmax Gumbel relaxations are provided for the argmax selection "
                                      "only; plain stochastic sampling is supported")
        codes = self.effective_codes()
        h, m, _ = flat.shape
        x = flat.float()
        temperature = g.get("temperature", 1.0)
        seed = gumbel_mod.draw_seed(flat.device)  # once per call, whichever path runs
        ind = None
        fused = getattr(search.get_backend(), "sample_codes", None)
        if fused is not None and not os.environ.get("VQ_NO_FUSED_SAMPLE"):  # (read per call: tests compare both paths)
            packed = self.packed_codes()
            ind = fused(x.detach(), codes.detach(), metric=self.metric, tau=1.0 / temperature, seed=seed,
                        **({"packed": packed} if packed is not None else {}))
        if ind is None:  # rows wider than 512 dims, a backend without the sweep, or the switch
            step = losses._rows_per_chunk(h, self.codebook_size)
            ind = torch.empty((h, m), dtype=torch.int64, device=flat.device)
            eps = 1e-5  # the reference's log(t) clamps at 1e-5 (utils/general.py:25-26)
            with torch.no_grad():
                for r0 in range(0, m, step):
                    sims = losses.similarity_matrix(x[:, r0:r0 + step].detach(), codes.detach(), self.metric)
                    noise = torch.zeros_like(sims).uniform_(0, 1)
                    gumbel = -(-noise.clamp(min=eps).log()).clamp(min=eps).log()
                    ind[:, r0:r0 + step] = (sims / temperature + gumbel).argmax(dim=-1)
        if idx is not None:
            idx.copy_(ind[..., None])
        picked = codes[torch.arange(h, device=flat.device)[:, None], ind]  # [h, m, d]; differentiable w.r.t. a learnable codebook
        sq_err = None
        if want_sq_err:
            target = picked if codebook_grad_from_err else picked.detach()
            sq_err = ((target - x) ** 2).sum(dtype=torch.float64).reshape(1)
        if ste and rotate:
            out = search.rotate_ste(x, picked)
        else:
            out = x + (picked - x).detach() if ste else picked
        return out, ind, sq_err

    def similarities(self, flat: torch.Tensor) -> torch.Tensor:
        """The [h, M, K] matrix the reference returns on every call (codebooks.py:386,435), on demand
        (vq_similarities_f32: the very values the search compares).  The losses that consume it never ask for the
        whole matrix -- see losses.py."""
        from . import losses

        return losses.similarity_matrix(flat, self.effective_codes(), self.metric)

    def forward(self, x, mask=None, freeze_codebook=False, return_similarities=True):
        """(quantize, embed_ind, similarities) like the reference (codebooks.py:351,435).  A direct caller gets the full
        ``[h, ..., K]`` similarity tensor, as the reference returns it; pass ``return_similarities=False`` to skip its
        materialisation (the modules of this package never call this method: they use ``quantize_flat``)."""
        squeeze_head = x.ndim < 4
        x = x.float()
        if squeeze_head:
            x = x.unsqueeze(0)
        h, d = x.shape[0], x.shape[-1]
        lead = x.shape[1:-1]
        flat = x.reshape(h, -1, d)
        flat_mask = None
        if mask is not None:
            reps = flat.shape[1] // (mask.shape[0] * mask.shape[1])
            flat_mask = mask[:, None, :].expand(mask.shape[0], reps, mask.shape[1]).reshape(1, -1).expand(h, -1)

        if not self.is_initialized:
            self.seed_with_kmeans(flat, flat_mask)
            self.is_initialized = True

        if self.use_affine:
            self.update_affine(flat, flat_mask)

        out, idx, _ = self.quantize_flat(flat, frozen=freeze_codebook)
        sims = self.similarities(flat).reshape(h, *lead, self.codebook_size) if return_similarities else None

        if self.training and self.ema_update and not freeze_codebook:
            self.ema_step(flat.detach(), idx, flat_mask)

        quantize = out.reshape(h, *lead, d)
        embed_ind = idx.reshape(h, *lead)
        if squeeze_head:
            quantize, embed_ind = quantize[0], embed_ind[0]  # `sims` keeps the head dim, like the reference (codebooks.py:433)
        return quantize, embed_ind, sims

    # ------------------------------------------------------------------ training-state bookkeeping
    @torch.no_grad()
    def ema_step(self, flat: torch.Tensor, idx: torch.Tensor, flat_mask=None, sample_pool=None):
        """Exponential-moving-average codebook update + dead-code re-seeding (codebooks.py:399-426),
        expressed with index arithmetic instead of the reference's [h, M, K] one-hot products.
        ``sample_pool``: the rows re-seeding draws from, in the REFERENCE's row order (a tensor or a callable returning it;
        default ``flat``) -- the draw is an index into them, so the order matters (shared codebook with several heads)."""
        hits, sums = search.get_backend().ema_accumulate(flat, idx, self.codebook_size, flat_mask)
        if self.use_affine:
            # codebooks.py:400-403 sums the rows moved to the codebook's moments, (x - batch_mean) * r + codebook_mean with
            # r = codebook_std / batch_std.  Per code that is r * sum(x) + hits * (codebook_mean - batch_mean * r): the raw
            # rows are accumulated as always and the [h, K, D] result is corrected -- no transformed copy of [M, D]
            hits, sums = hits.contiguous(), sums.contiguous()
            fused = self._fused_affine("affine_apply")
            codebook_mean, codebook_variance, batch_mean, batch_variance = self._affine_now
            if fused is not None:
                sums = fused(sums, codebook_mean, codebook_variance, batch_mean, batch_variance, mode=1, hits=hits, out=sums)
            else:
                r = _affine_std(codebook_variance) / _affine_std(batch_variance)
                sums = sums * r + hits[..., None] * (codebook_mean - batch_mean * r)
        self.ema_apply(hits, sums)
        self.reseed_dead_codes(sample_pool if sample_pool is not None else flat)

    @torch.no_grad()
    def ema_apply(self, hits: torch.Tensor, sums: torch.Tensor):
        """Second half of the EMA step from ready statistics (hits [h, K], sums [h, K, D]): replica sync, lerp, Laplace
        smoothing, normalise -- codebooks.py:410-425."""
        hits, sums = hits.contiguous(), sums.contiguous()
        self._sync_sum(hits)
        self._sync_sum(sums)
        search.get_backend().ema_update(self.cluster_size.data, self.embed_avg.data, self.embeddings.data, hits, sums,
                                        decay=self.decay, eps=self.eps_for_smoothing,
                                        l2norm=self.weights_regularization is _unit_rows)
        self.invalidate_packed()

    @torch.no_grad()
    def ema_apply_shard(self, hits: torch.Tensor, sums: torch.Tensor, group, k_total: int):
        """EMA step of ONE SHARD of a codebook that is sharded over ``group`` (codebooks.py:410-425 for the codes this rank
        owns).  The statistics of a code live on its owner only, so they need no reduction; the Laplace smoothing
        normalises with the cluster sizes of the WHOLE codebook, so the per-shard totals are all-reduced."""
        w = 1.0 - self.decay
        self.cluster_size.data.lerp_(hits, w)
        self.embed_avg.data.lerp_(sums, w)
        total = self.cluster_size.data.sum(dim=-1, keepdim=True)
        dist.all_reduce(total, group=group)
        smoothed = (self.cluster_size.data + self.eps_for_smoothing) / (total + k_total * self.eps_for_smoothing) * total
        fresh = self.weights_regularization(self.embed_avg.data / smoothed[..., None])
        self.embeddings.data.copy_(fresh)
        self.invalidate_packed()

    def _expire_on_device(self, flat, sharded: bool = False):
        """reseed_dead_codes with ``expire_on_device``: one seed from torch's generator (on the device), then the backend's
        launches, issued whether or not a code expired -- no ``.any()``, no ``.item()``, nothing the host waits for."""
        from . import gumbel

        if sharded or (self.use_ddp and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            raise NotImplementedError("expire_on_device draws the replacement rows on each device for itself: replicas (use_ddp) "
                                      "and the shards of a sharded codebook would not stay identical; turn it off for them")
        expire = getattr(search.get_backend(), "expire_codes", None)
        if expire is None:
            raise RuntimeError("expire_on_device needs a backend with the native expiry kernel (expire_codes)")
        pool, chain, stage = None, None, 0
        if isinstance(flat, tuple):  # (x [M, D], stage codes [Q | 1, K, D], idx [M, Q], q): the residual r_q is never made
            x, codes, idx, stage = flat
            chain = (x if x.dtype == torch.float32 else x.float(), codes.contiguous(), idx)
        else:
            pool = flat() if callable(flat) else flat
            if pool.dtype != torch.float32:
                pool = pool.float()
            if pool.stride(-1) != 1 and pool.shape[-1] != 1:
                pool = pool.contiguous()
        seed = gumbel.draw_seed(self.embeddings.device)
        expire(self.cluster_size.data, self.embed_avg.data, self.embeddings.data, pool, chain=chain, stage=stage,
               threshold=self.threshold_ema_dead_code, reset_cluster_size=self.reset_cluster_size,
               l2norm=self.weights_regularization is _unit_rows, seed=seed)
        self.invalidate_packed()

    @torch.no_grad()
    def reseed_dead_codes(self, flat, sharded: bool = False):
        """``flat`` [h, M, D], or a callable producing it (evaluated only if some code actually expired).  With
        ``expire_on_device`` also a residual chain (x [M, D], codes [Q | 1, K, D], idx [M, Q], stage), and the whole step is
        left to the device (see _expire_on_device); ``sharded``: the codebook is one shard of a larger one."""
        if self.threshold_ema_dead_code == 0:
            return
        if self.expire_on_device:
            return self._expire_on_device(flat, sharded)
        dead = self.cluster_size < self.threshold_ema_dead_code
        if not bool(dead.any()):
            return
        if callable(flat):
            flat = flat()
        pool = self.weights_regularization(flat)
        for head in range(pool.shape[0]):
            n_dead = int(dead[head].sum().item())
            if n_dead == 0:
                continue
            kmeans_sync = (self.kmeans_params or {}).get("sync", True)
            spread = self.use_ddp and dist.is_available() and dist.is_initialized()
            if spread and kmeans_sync and self.distributed_replace_codes:
                picked = _pick_rows_all_ranks(pool[head], n_dead)  # the same replacement vectors on every replica
            else:
                picked = _pick_rows(pool[head], n_dead)
                if spread and not self.distributed_replace_codes:  # codebooks.py:236-237: average the replicas' draws
                    dist.all_reduce(picked)
                    picked = picked / dist.get_world_size()
            self.embeddings.data[head][dead[head]] = picked
            self.invalidate_packed()
            self.cluster_size.data[head][dead[head]] = self.reset_cluster_size
            self.embed_avg.data[head][dead[head]] = picked * self.reset_cluster_size

    @torch.no_grad()
    def seed_with_kmeans(self, flat: torch.Tensor, flat_mask=None):
        """Lloyd iterations on the first batch (utils/kmeans.py:38-120); the assignment step is the
        native search kernel."""
        if flat_mask is not None:
            h = flat.shape[0]
            flat = flat[flat_mask].reshape(h, -1, flat.shape[-1])
        h, m, d = flat.shape
        k = self.codebook_size
        iters = (self.kmeans_params or {}).get("iter", 10)
        sync = self.use_ddp and (self.kmeans_params or {}).get("sync", True)
        # utils/kmeans.py:82-118: the first centroids are RAW sampled rows and the per-cluster means are means of the RAW rows;
        # with the cosine similarity only the new centroids are L2-normalised (the rows are not, unless the module's
        # transform_input already did it)
        data = flat
        pick = _pick_rows_all_ranks if (sync and dist.is_available() and dist.is_initialized()) else _pick_rows
        means = torch.stack([pick(data[i], k) for i in range(h)])
        counts = torch.zeros((h, k), dtype=flat.dtype, device=flat.device)
        for _ in range(iters):
            idx, _best, _ = search.nearest_with_distance(data, means, metric=self.metric)
            counts, sums = search.get_backend().ema_accumulate(data.contiguous(), idx.contiguous(), k)
            if sync and dist.is_initialized():
                dist.all_reduce(counts)
                dist.all_reduce(sums)
            fresh = sums / counts.clamp(min=1.0)[..., None]
            if self.use_cosine_sim:
                fresh = _unit_rows(fresh)
            means = torch.where((counts == 0)[..., None], means, fresh)
        self.embeddings.data.copy_(means)
        self.invalidate_packed()
        self.embed_avg.data.copy_(means * counts[..., None])
        self.cluster_size.data.copy_(counts)
