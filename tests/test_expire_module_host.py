"""CPU: the host side of dead-code expiry on the device -- the switch, what it refuses, and that the step traces through
torch.ops.vq_mi355x.expire_codes without a graph break (dynamo with fake tensors: nothing executes)."""
from __future__ import annotations

import pytest
import torch


def _codebook(**kw):
    from vector_quantization.codebook import Codebook

    torch.manual_seed(0)
    return Codebook(dim=8, codebook_size=16, **kw)


def test_the_switch_is_a_plain_attribute_set_per_codebook():
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    rvq = vq.ResidualVQ(dim=8, num_quantizers=3, codebook_params=CodebookParams(dim=8, codebook_size=16))
    books = [layer._codebook for layer in rvq.layers]
    assert all(b.expire_on_device is False for b in books)
    keys = set(rvq.state_dict())
    assert vq.set_expire_on_device(rvq) is rvq and all(b.expire_on_device is True for b in books)
    assert set(rvq.state_dict()) == keys and not any("expire" in k for k in keys)
    vq.set_expire_on_device(rvq, False)
    assert not any(b.expire_on_device for b in books)
    assert "expire_on_device" not in {f.name for f in __import__("dataclasses").fields(CodebookParams)}
    assert "set_expire_on_device" in vq.__all__ and "GraphedTrainForward" in vq.__all__


def test_no_threshold_no_step():
    cb = _codebook(threshold_ema_dead_code=0)
    cb.expire_on_device = True
    cb.reseed_dead_codes(lambda: pytest.fail("the pool was evaluated although expiry is off"))


def test_cpu_tensors_fail_loudly_there_is_no_fallback():
    from vector_quantization import native

    cb = _codebook()
    cb.expire_on_device = True
    with pytest.raises(native.NativeUnavailable):
        cb.reseed_dead_codes(torch.randn(1, 30, 8))


def test_replicas_and_shards_are_refused(monkeypatch):
    from vector_quantization import codebook as codebook_mod

    class World:
        is_available = staticmethod(lambda: True)
        is_initialized = staticmethod(lambda: True)
        get_world_size = staticmethod(lambda group=None: 2)

    cb = _codebook(use_ddp=True)
    cb.expire_on_device = True
    monkeypatch.setattr(codebook_mod, "dist", World)
    with pytest.raises(NotImplementedError, match="expire_on_device"):
        cb.reseed_dead_codes(torch.randn(1, 30, 8))
    monkeypatch.undo()
    single = _codebook()
    single.expire_on_device = True
    with pytest.raises(NotImplementedError, match="expire_on_device"):
        single.reseed_dead_codes(torch.randn(1, 30, 8), sharded=True)


def test_graphed_train_forward_checks_mode_and_switch_before_anything_else():
    import vector_quantization as vq
    from vector_quantization.codebooks import CodebookParams

    mod = vq.VectorQuantize(dim=8, codebook_params=CodebookParams(dim=8, codebook_size=16))
    x = torch.randn(2, 5, 8)
    with pytest.raises(ValueError, match="expire_on_device"):
        vq.GraphedTrainForward(mod.train(), x)
    vq.set_expire_on_device(mod)
    with pytest.raises(ValueError, match=r"module\.train\(\)"):
        vq.GraphedTrainForward(mod.eval(), x)
    with pytest.raises(ValueError, match="device tensor"):
        vq.GraphedTrainForward(mod.train(), x)
    with pytest.raises(ValueError, match="GraphedTrainForward"):  # the inference wrapper points at the training one
        vq.GraphedForward(mod.train(), x)


@pytest.mark.parametrize("pool", ["tensor", "callable", "chain"])
def test_the_step_traces_through_the_registered_op(pool):
    import torch._dynamo as dynamo

    import vector_quantization as vq

    cb = vq.set_expire_on_device(_codebook())

    def step(x, codes, idx):
        cb.reseed_dead_codes({"tensor": x[None], "callable": lambda: x[None], "chain": (x, codes, idx, 1)}[pool])
        return cb.embeddings + 0

    dynamo.reset()
    with torch.no_grad():
        gm, _guards = dynamo.export(step)(torch.randn(30, 8), torch.randn(3, 16, 8), torch.randint(0, 16, (30, 3)))
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert any("vq_mi355x.expire_codes" in t for t in targets), targets
    assert any("randint" in t for t in targets), "the seed is not drawn inside the graph"
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        picked = torch.ops.vq_mi355x.expire_codes(torch.empty(2, 16), torch.empty(2, 16, 8), torch.empty(2, 16, 8), torch.empty(2, 30, 8),
                                                  None, None, None, 0, 2.0, 2.0, False, torch.empty(2, dtype=torch.int64))
        assert picked.shape == (2, 16) and picked.dtype == torch.int64
