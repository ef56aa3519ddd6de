"""GPU: dead-code expiry on the device through the modules (Codebook.expire_on_device, set_expire_on_device,
GraphedTrainForward).  Every test here needs the switch, which the code before it does not have.

The rows are train_dense.exact_inputs-style (integers in [-15, 15] times 2^-3; for the cosine case four entries of +-1, whose
normalisation is exact as well), so the EMA sums are the same bits in any order and a module with the mode on can be compared
bit for bit with clones that run the host path or no expiry at all."""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _native_backend():
    from vector_quantization import native, search

    native.load()
    search.set_backend(None)
    yield


def _grid_rows(shape, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.integers(-15, 16, shape).astype(np.float32) * np.float32(0.125))).to(DEV)


def _unit_rows(shape, seed):
    """Rows with four entries of +-1: their l2 norm is 2 and the normalised row +-0.5, exact in fp32."""
    rng = np.random.default_rng(seed)
    x = np.zeros(shape, dtype=np.float32).reshape(-1, shape[-1])
    for row in x:
        row[rng.choice(shape[-1], 4, replace=False)] = rng.choice([-1.0, 1.0], 4)
    return torch.from_numpy(x.reshape(shape)).to(DEV)


def _vq(K=300, dim=32, **kw):
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    cb = dict(dim=dim, codebook_size=K, threshold_ema_dead_code=2)
    cb.update(kw.pop("cb", {}))
    torch.manual_seed(1234)
    return vq.VectorQuantize(dim=dim, codebook_params=CodebookParams(**cb), **kw).to(DEV).train()


def _books(mod):
    from vector_quantization.codebook import Codebook

    return [m for m in mod.modules() if isinstance(m, Codebook)]


def _without_expiry(mod):
    twin = copy.deepcopy(mod)
    for b in _books(twin):
        b.threshold_ema_dead_code = 0
        b.expire_on_device = False
    return twin


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _check_codebook(book, plain, pools, what=""):
    """``book``: a Codebook after one step with the mode on; ``plain``: its clone after the same step without expiry (its
    cluster sizes name the dead codes); ``pools``: per head the [N, D] rows a new code may be (already transformed)."""
    dead = plain.cluster_size < book.threshold_ema_dead_code
    live = ~dead
    for name in ("cluster_size", "embed_avg", "embeddings"):
        assert torch.equal(_bits(getattr(book, name))[live], _bits(getattr(plain, name))[live]), f"{what}: live {name} changed"
    reset = torch.tensor(float(book.reset_cluster_size), device=DEV)
    total = 0
    for h in range(dead.shape[0]):
        ks = torch.nonzero(dead[h])[:, 0]
        pool = pools[h if len(pools) > 1 else 0]
        assert len(torch.unique(pool, dim=0)) == len(pool), "the test's pool has equal rows: a code would not name its row"
        new = book.embeddings[h, ks]
        same = (_bits(new)[:, None, :] == _bits(pool)[None, :, :]).all(dim=-1)  # [n_dead, N]
        assert bool((same.sum(dim=1) == 1).all()), f"{what}: a re-seeded code of head {h} is no row of the pool"
        rows = same.int().argmax(dim=1)
        if len(ks) <= len(pool):
            assert len(torch.unique(rows)) == len(ks), f"{what}: head {h} took a row twice although there were enough"
        assert bool((book.cluster_size[h, ks] == reset).all())
        assert torch.equal(_bits(book.embed_avg[h, ks]), _bits(new * reset))
        total += len(ks)
    return total


VARIANTS = {
    "plain": dict(),
    "cosine-l2norm": dict(cb=dict(use_cosine_sim=True, transform_input="l2norm", weights_regularization="l2norm")),
    "heads-shared": dict(heads=2, codebook_dim=16, cb=dict(dim=16)),
    "heads-separate": dict(heads=2, codebook_dim=16, separate_codebook_per_head=True, cb=dict(dim=16)),
    "mask": dict(),
    "affine": dict(),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_one_training_forward_with_the_mode_on(variant):
    import vector_quantization as vq
    from vector_quantization.codebooks import AffineParameters

    kw = copy.deepcopy(VARIANTS[variant])
    if variant == "affine":
        kw["cb"] = dict(use_affine=True, affine_params=AffineParameters(sync=False))
    mod = _vq(**kw)
    x = _unit_rows((4, 64, 32), 5) if variant == "cosine-l2norm" else _grid_rows((4, 64, 32), 5)
    fwd = dict(mask=(torch.arange(64, device=DEV)[None, :] < torch.tensor([64, 40, 64, 10], device=DEV)[:, None])) \
        if variant == "mask" else {}
    host, plain = copy.deepcopy(mod), _without_expiry(mod)
    vq.set_expire_on_device(mod)
    assert all(b.expire_on_device for b in _books(mod)) and not any(b.expire_on_device for b in _books(host))
    assert "expire_on_device" not in mod.state_dict() and not any("expire" in k for k in mod.state_dict())
    outs = []
    for m in (mod, host, plain):
        torch.manual_seed(99)
        with torch.no_grad():
            outs.append(m(x, **fwd))
    torch.cuda.synchronize()
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b), "the forward's outputs depend on the expiry mode"
    rows = F.normalize(x, dim=-1) if variant == "cosine-l2norm" else x
    if variant == "heads-shared":
        pools = [rows.reshape(-1, 16)]
    elif variant == "heads-separate":
        pools = [rows.reshape(-1, 2, 16)[:, h] for h in range(2)]
    else:
        pools = [rows.reshape(-1, 32)]
    book = mod._codebook
    n = _check_codebook(book, plain._codebook, pools, variant)
    assert n >= 40 * book.num_codebooks, "the case is about dying codes"
    # the host path's live codes are the same bits; its new codes are rows of the same pool (drawn by torch's generator)
    dead = plain._codebook.cluster_size < 2
    assert torch.equal(_bits(host._codebook.embeddings)[~dead], _bits(book.embeddings)[~dead])
    _check_codebook(host._codebook, plain._codebook, pools, variant + " (host path)")


def _rvq(groups=None):
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    torch.manual_seed(4321)
    if groups:
        return vq.GroupedResidualVQ(dim=32 * groups, groups=groups, num_quantizers=3,
                                    codebook_params=CodebookParams(dim=32, codebook_size=128)).to(DEV).train()
    return vq.ResidualVQ(dim=32, num_quantizers=3, codebook_params=CodebookParams(dim=32, codebook_size=128)).to(DEV).train()


@pytest.mark.parametrize("groups", [None, 2], ids=["ResidualVQ", "GroupedResidualVQ"])
def test_residual_stacks_reseed_from_their_stage_residual_without_the_chain(groups, monkeypatch):
    import vector_quantization as vq
    from vector_quantization import residual

    chain_of = residual._residual_chain
    mod = _rvq(groups)
    G = groups or 1
    x = _grid_rows((4, 64, 32 * G), 6)
    plain = _without_expiry(mod)
    vq.set_expire_on_device(mod)
    stacks = list(mod.rvqs) if groups else [mod]
    before = [torch.stack([layer._codebook.embeddings.detach()[0].clone() for layer in rvq.layers]) for rvq in stacks]

    def no_chain(*a, **k):
        raise AssertionError("_residual_chain was materialised although the codebooks expire on the device")

    monkeypatch.setattr(residual, "_residual_chain", no_chain)
    fused, fused_forward = [], mod._forward_fused
    monkeypatch.setattr(mod, "_forward_fused", lambda *a, **k: (fused.append(1), fused_forward(*a, **k))[1])
    with torch.no_grad():
        _, idx, _ = mod(x)
        plain(x)
    torch.cuda.synchronize()
    assert fused, "the stack did not take its fused path"
    idx = idx if groups else idx[None]  # [G, b, n, Q]
    reseeded = 0
    for g, rvq in enumerate(stacks):
        xg = x.reshape(-1, G, 32)[:, g]
        chain = chain_of(xg, before[g], idx[g].reshape(-1, 3), ste=True)
        plain_rvq = plain.rvqs[g] if groups else plain
        for q, layer in enumerate(rvq.layers):
            book, ref = layer._codebook, plain_rvq.layers[q]._codebook
            dead = ref.cluster_size < 2
            ks = torch.nonzero(dead[0])[:, 0]
            new = book.embeddings[0, ks]
            same = (_bits(new)[:, None, :] == _bits(chain[q])[None, :, :]).all(dim=-1)
            assert bool(same.any(dim=1).all()), f"group {g} stage {q}: a re-seeded code is no row of r_{q}"
            assert bool((book.cluster_size[0, ks] == 2.0).all()) and torch.equal(_bits(book.embed_avg[0, ks]), _bits(new * 2.0))
            assert bool((book.cluster_size[0][~dead[0]] >= 2.0).all())
            reseeded += len(ks)
    assert reseeded >= 3 * G * 10, "the case is about dying codes"


# ---------------------------------------------------------------------------------------------------- no synchronisation
def _balanced(seed):
    """256 rows of dim 8 around four far-apart centres, 64 each: every code keeps its rows, nothing expires."""
    centres = 16.0 * torch.eye(4, 8, device=DEV)
    return (centres[torch.arange(256, device=DEV) % 4] + _grid_rows((256, 8), seed)).reshape(4, 64, 8)


def test_graphed_train_forward_equals_eager_steps():
    import vector_quantization as vq

    mod = _vq(K=4, dim=8)
    with torch.no_grad():
        mod._codebook.embeddings.copy_(16.0 * torch.eye(4, 8, device=DEV)[None])
        mod._codebook.embed_avg.copy_(mod._codebook.embeddings)
    vq.set_expire_on_device(mod)
    twin = copy.deepcopy(mod)
    example = _balanced(70)
    step = vq.GraphedTrainForward(mod, example, warmup=2)
    with torch.no_grad():
        for _ in range(2):
            twin(example)
    for i in range(3):
        x = _balanced(71 + i)
        q, idx, loss = step(x)
        with torch.no_grad():
            tq, tidx, tloss = twin(x)
        assert torch.equal(q, tq) and torch.equal(idx, tidx) and torch.equal(loss, tloss)
        for name in ("embeddings", "cluster_size", "embed_avg"):
            assert torch.equal(_bits(getattr(mod._codebook, name)), _bits(getattr(twin._codebook, name))), (i, name)
    assert bool((mod._codebook.cluster_size >= 2).all()), "the case is about a codebook in which nothing expires"


def test_graphed_train_forward_expires_codes_at_replay_time():
    import vector_quantization as vq

    mod = _vq()
    vq.set_expire_on_device(mod)
    step = vq.GraphedTrainForward(mod, _grid_rows((4, 64, 32), 80), warmup=2)
    for i in range(3):
        x = _grid_rows((4, 64, 32), 81 + i)
        plain = _without_expiry(mod)
        step(x)
        with torch.no_grad():
            plain(x)
        torch.cuda.synchronize()
        n = _check_codebook(mod._codebook, plain._codebook, [x.reshape(-1, 32)], f"replay {i}")
        assert n >= 40


def test_forward_and_backward_under_one_graph():
    import vector_quantization as vq

    torch.manual_seed(11)
    lin = torch.nn.Linear(32, 32).to(DEV)
    mod = _vq(commitment_weight=0.25)
    vq.set_expire_on_device(mod)
    x = torch.randn(4, 64, 32, device=DEV).requires_grad_(True)

    def step(lin, mod, x):
        q, _, loss = mod(lin(x))
        (q.square().sum() + loss.sum()).backward()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(lin, mod, x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for m in mod.modules():
        if hasattr(m, "invalidate_packed"):
            m.invalidate_packed()
    lin.zero_grad(set_to_none=True)
    x.grad = None
    twin_lin, twin, tx = copy.deepcopy(lin), copy.deepcopy(mod), x.detach().clone().requires_grad_(True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(lin, mod, x)
    for m in mod.modules():
        if hasattr(m, "invalidate_packed"):
            m.invalidate_packed()
    graph.replay()
    step(twin_lin, twin, tx)
    torch.cuda.synchronize()
    assert x.grad is not None and bool(x.grad.any())
    assert torch.equal(x.grad, tx.grad)
    assert torch.equal(lin.weight.grad, twin_lin.weight.grad) and torch.equal(lin.bias.grad, twin_lin.bias.grad)


# ------------------------------------------------------------------------------------------------------------- guards
def test_replicas_are_refused(monkeypatch):
    import vector_quantization as vq
    from vector_quantization import codebook as codebook_mod

    class World:
        @staticmethod
        def is_available():
            return True

        @staticmethod
        def is_initialized():
            return True

        @staticmethod
        def get_world_size(group=None):
            return 2

        @staticmethod
        def all_reduce(t, *a, **k):
            return None

    mod = _vq(sync_codebook=True)
    assert mod._codebook.use_ddp
    vq.set_expire_on_device(mod)
    monkeypatch.setattr(codebook_mod, "dist", World)
    with pytest.raises(NotImplementedError, match="expire_on_device"), torch.no_grad():
        mod(_grid_rows((4, 64, 32), 90))
    with pytest.raises(NotImplementedError, match="expire_on_device"):
        mod._codebook.reseed_dead_codes(_grid_rows((1, 64, 32), 91), sharded=True)
    torch.cuda.synchronize()


def test_graphed_train_forward_needs_the_switch_and_train_mode():
    import vector_quantization as vq

    mod = _vq()
    x = _grid_rows((4, 64, 32), 92)
    with pytest.raises(ValueError, match="expire_on_device"):
        vq.GraphedTrainForward(mod, x)
    vq.set_expire_on_device(mod)
    with pytest.raises(ValueError, match="train"):
        vq.GraphedTrainForward(mod.eval(), x)
    vq.set_expire_on_device(mod, False)
    assert not mod._codebook.expire_on_device


def _reseed_before_the_switch(self, flat):
    """Codebook.reseed_dead_codes as it was before expire_on_device existed (single process), statement for statement."""
    from vector_quantization.codebook import _pick_rows

    if self.threshold_ema_dead_code == 0:
        return
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
        picked = _pick_rows(pool[head], n_dead)
        self.embeddings.data[head][dead[head]] = picked
        self.invalidate_packed()
        self.cluster_size.data[head][dead[head]] = self.reset_cluster_size
        self.embed_avg.data[head][dead[head]] = picked * self.reset_cluster_size


def test_the_default_consumes_torchs_generator_as_before(monkeypatch):
    mod = _vq()
    assert mod._codebook.expire_on_device is False
    twin = copy.deepcopy(mod)
    monkeypatch.setattr(twin._codebook, "reseed_dead_codes", lambda flat: _reseed_before_the_switch(twin._codebook, flat))
    x = _grid_rows((4, 64, 32), 93)
    states = []
    for m in (mod, twin):
        torch.manual_seed(2024)
        with torch.no_grad():
            m(x)
        torch.cuda.synchronize()
        states.append(torch.cuda.get_rng_state(DEV))
    assert torch.equal(states[0], states[1])
    for name in ("embeddings", "cluster_size", "embed_avg"):
        assert torch.equal(_bits(getattr(mod._codebook, name)), _bits(getattr(twin._codebook, name)))
    torch.manual_seed(2024)
    assert not torch.equal(torch.cuda.get_rng_state(DEV), states[0]), "the step drew nothing: the case is about dying codes"
