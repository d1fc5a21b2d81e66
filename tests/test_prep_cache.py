"""The host mechanics of the derived-weight caches, without a GPU: no cached, folded weight may outlive an edit of its source.

ops.split_rows_weight (the global ops._SPLIT_CACHE) against ops.pack_w1_split of the values the tensor holds NOW: in-place edits, the death of
the tensor, views of a shared storage, views that differ in strides alone, tensors made under torch.inference_mode().  _PrepCache (the per-module
folded weights of laud_resnet / laud_regnet) on a Masker_spatial and a two-layer Masker_channel_MLP, whose preparation is plain torch: every
way an edit arrives drops the cache, and the two documented blind spots (an edit through `p.data`, a replaced parameter object) are shown to
be blind -- the negative controls that prove the assertions of this file can fail.  The whole-model half of this is tests/test_hip_weight_caches.py."""
import gc

import pytest
import torch
import torch.nn as nn

from fill import seeded_randn


@pytest.fixture
def ops():
    from laudnet_amd import ops
    ops._SPLIT_CACHE.clear()
    yield ops
    ops._SPLIT_CACHE.clear()


def _want(ops, w):
    """the split of the values w holds now, computed from a private copy"""
    w2 = w.detach().clone().float().reshape(w.shape[0], -1)
    return ops.pack_w1_split(w2)


def _check(ops, w, what=""):
    got = ops.split_rows_weight(w)
    want = _want(ops, w)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(got, want), f"{what}: split_rows_weight returned the split of other values"
    return got


# ------------------------------------------------------------------------------------------------ ops.split_rows_weight
def test_split_follows_in_place_edits_and_keeps_one_entry(ops):
    w = seeded_randn((24, 1, 32), 1)
    first = _check(ops, w, "first call")
    assert ops.split_rows_weight(w) is first, "an unchanged tensor must hit the cache"
    n0 = len(ops._SPLIT_CACHE)
    assert n0 == 1
    for r in range(20):
        old_keys = set(ops._SPLIT_CACHE)
        with torch.no_grad():
            w.mul_(1.25) if r % 2 else w.add_(0.125 * (r + 1))
        got = _check(ops, w, f"round {r}")
        assert got is not first
        assert not (old_keys & set(ops._SPLIT_CACHE)), f"round {r}: the entry of the older version is still cached"
        assert len(ops._SPLIT_CACHE) == n0, f"round {r}: {len(ops._SPLIT_CACHE)} entries for one tensor"


def test_split_entry_dies_with_its_tensor(ops):
    w = seeded_randn((8, 16), 2)
    _check(ops, w)
    assert len(ops._SPLIT_CACHE) == 1
    del w
    gc.collect()
    assert len(ops._SPLIT_CACHE) == 0, "the entry outlived its tensor: a later tensor at the same address would be served its split"


def test_split_of_a_view_sees_edits_through_the_base_and_lives_as_long_as_the_base(ops):
    base = seeded_randn((8, 1, 16), 3)
    v = base[2:6]
    _check(ops, v, "view")
    with torch.no_grad():
        base.mul_(-3.0)                      # an edit through the base ...
    _check(ops, v, "view after an edit of its base")       # ... is seen through the view
    assert len(ops._SPLIT_CACHE) == 1
    del v
    gc.collect()
    assert len(ops._SPLIT_CACHE) == 1, "callers pass throw-away views: the entry belongs to the tensor that owns the storage"
    _check(ops, base[2:6], "a new view of the same rows")
    assert len(ops._SPLIT_CACHE) == 1
    del base
    gc.collect()
    assert len(ops._SPLIT_CACHE) == 0


def test_split_tells_views_that_differ_in_strides_alone(ops):
    """Same storage, same address, same shape [2, 1, 16], different strides: rows 0, 1 against rows 0, 2 of base."""
    base = seeded_randn((4, 1, 16), 4)
    a = base[:2]
    b = base.view(2, 2, 16)[:, :1, :]
    assert a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() != b.stride()
    assert not torch.equal(a, b)
    for rnd in range(2):                     # (second round: both served from the cache)
        _check(ops, a, f"contiguous view, round {rnd}")
        _check(ops, b, f"strided view, round {rnd}")
    _check(ops, a, "contiguous view again")
    assert len(ops._SPLIT_CACHE) == 2
    with torch.no_grad():
        base.add_(1.0)
    _check(ops, b, "strided view after an edit")
    _check(ops, a, "contiguous view after an edit")
    assert len(ops._SPLIT_CACHE) == 2
    del a, b, base
    gc.collect()
    assert len(ops._SPLIT_CACHE) == 0


def test_split_of_an_inference_tensor(ops):
    """A tensor made under torch.inference_mode() has no version counter (reading ._version raises): the folded weights of a first forward
    under inference_mode are such tensors."""
    with torch.inference_mode():
        w = nn.Parameter(seeded_randn((16, 24), 5)).detach().reshape(16, 1, 24).float().contiguous()
    assert w.is_inference()
    with pytest.raises(RuntimeError):
        w._version
    for ctx in (torch.inference_mode, torch.no_grad):       # a cache built under one context serves the other
        with ctx():
            first = _check(ops, w, ctx.__name__)
            assert ops.split_rows_weight(w) is first, "the second call must hit the cache"
    assert len(ops._SPLIT_CACHE) == 1
    del w, first
    gc.collect()
    assert len(ops._SPLIT_CACHE) == 0


def test_tensor_version_and_version_key(ops):
    a = torch.ones(3)
    with torch.inference_mode():
        b = torch.ones(3)
    assert ops.tensor_version(a) == a._version == 0 and ops.tensor_version(b) == -1
    steps = ops._OPTIMIZER_STEPS[0]
    assert ops.version_key([a, b]) == ((a.data_ptr(), 0), (b.data_ptr(), -1), steps)
    a.add_(1.0)
    assert ops.tensor_version(a) == 1 and ops.version_key((a,)) == ((a.data_ptr(), 1), steps)


@pytest.mark.parametrize("fused", [False, True])
def test_split_follows_optimizer_steps(ops, fused):
    """The fused optimizer implementations update a parameter WITHOUT bumping its version counter: the keys carry a count of optimizer steps."""
    w = nn.Parameter(seeded_randn((8, 1, 16), 6))
    alias = w.detach().reshape(8, 1, 16).float().contiguous()       # what a module's preparation keeps of an fp32 weight: the same storage
    assert alias.data_ptr() == w.data_ptr()
    _check(ops, alias, "before the step")
    key = ops.version_key([w])
    for cls in (torch.optim.SGD, torch.optim.AdamW):
        w.grad = seeded_randn((8, 1, 16), 7)
        version = w._version
        cls([w], lr=0.1, fused=fused).step()
        assert fused == (w._version == version), "torch's fused steps have begun to bump version counters (or the plain ones stopped)"
        assert ops.version_key([w]) != key
        key = ops.version_key([w])
        _check(ops, alias, f"after {cls.__name__}(fused={fused}).step()")
        assert len(ops._SPLIT_CACHE) == 1


# ------------------------------------------------------------------------------------------------ _PrepCache
def _spatial():
    from laudnet_amd.laud_resnet import Masker_spatial
    m = Masker_spatial(24, 1, 7).eval()
    with torch.no_grad():
        m.conv.weight.copy_(seeded_randn(tuple(m.conv.weight.shape), 11))
        m.conv.bias.copy_(seeded_randn(tuple(m.conv.bias.shape), 12))
    return m


def _mlp():
    from laudnet_amd.laud_resnet import Masker_channel_MLP
    m = Masker_channel_MLP(24, 16, layers=2, reduction=16).eval()
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.copy_(seeded_randn(tuple(p.shape), 21 + i))
    return m


def _prep(m):
    return m._wb() if hasattr(m, "_wb") else m._weights()


def _expected(m):
    """what the preparation must hold, from the parameters as they are now (float64 copies: nothing here aliases the module)"""
    if hasattr(m, "_wb"):
        src = (m.conv.weight.reshape(m.conv.weight.shape[0], -1), m.conv.bias)
    else:
        src = (m.conv[0].weight, m.conv[0].bias, m.conv[2].weight, m.conv[2].bias)
    return tuple(t.detach().double().clone() for t in src)


def _assert_prep(m, what):
    prep = _prep(m)
    want = _expected(m)
    assert m._cache_valid(), what
    assert len(prep) == len(want)
    for i, (g, w) in enumerate(zip(prep, want)):
        assert g.dtype == torch.float32 and g.shape == w.shape, f"{what}: prepared tensor {i}"
        assert torch.equal(g.double(), w), f"{what}: prepared tensor {i} does not hold the parameter's values"
    return prep


def _set_grads(m, seed):
    for i, p in enumerate(m.parameters()):
        p.grad = seeded_randn(tuple(p.shape), seed + i)


def _edit_mul(m, p):
    with torch.no_grad():
        p.mul_(1.5)


def _edit_copy(m, p):
    with torch.no_grad():
        p.copy_(seeded_randn(tuple(p.shape), 31))


def _edit_sgd(m, p):
    _set_grads(m, 41)
    torch.optim.SGD(m.parameters(), lr=0.1).step()


def _edit_adamw(m, p):
    _set_grads(m, 51)
    torch.optim.AdamW(m.parameters(), lr=0.1).step()


def _edit_sgd_fused(m, p):        # (the fused implementations do not bump the parameters' version counters)
    _set_grads(m, 71)
    torch.optim.SGD(m.parameters(), lr=0.1, fused=True).step()


def _edit_adamw_fused(m, p):
    _set_grads(m, 81)
    torch.optim.AdamW(m.parameters(), lr=0.1, fused=True).step()


def _new_state(m):
    return {k: v.detach().clone() * 1.5 + 0.25 for k, v in m.state_dict().items()}


def _edit_load(m, p):
    m.load_state_dict(_new_state(m))


def _edit_load_assign(m, p):
    m.load_state_dict(_new_state(m), assign=True)


def _edit_dtype_round_trip(m, p):
    m.to(torch.float64).to(torch.float32)


def _edit_train_eval(m, p):
    m.train()
    m.eval()


def _edit_invalidate(m, p):
    m.invalidate()


EDITS = {"mul_": _edit_mul, "copy_": _edit_copy, "sgd_step": _edit_sgd, "adamw_step": _edit_adamw, "sgd_fused_step": _edit_sgd_fused,
         "adamw_fused_step": _edit_adamw_fused, "load_state_dict": _edit_load,
         "load_state_dict_assign": _edit_load_assign, "dtype_round_trip": _edit_dtype_round_trip, "train_eval": _edit_train_eval,
         "invalidate": _edit_invalidate}
PER_PARAMETER = ("mul_", "copy_")       # in-place edits of ONE tensor: tried on every parameter in turn (a key that forgets one)


@pytest.mark.parametrize("edit", sorted(EDITS))
@pytest.mark.parametrize("make", [_spatial, _mlp], ids=["spatial", "mlp"])
def test_prep_cache_is_dropped_by_every_edit(make, edit):
    n = len(list(make().parameters())) if edit in PER_PARAMETER else 1
    for which in range(n):
        m = make()
        _assert_prep(m, "first preparation")
        assert _prep(m) is m._prep and m._cache_valid(), "a second call must be a hit"
        before = _expected(m)
        EDITS[edit](m, list(m.parameters())[which])
        assert not m._cache_valid(), f"{edit} on parameter {which}: the cache still counts as valid"
        _assert_prep(m, f"after {edit} on parameter {which}")
        changed = any(not torch.equal(a, b) for a, b in zip(before, _expected(m)))
        assert changed == (edit not in ("dtype_round_trip", "train_eval", "invalidate")), "the edit itself is not what this test says it is"


@pytest.mark.parametrize("make", [_spatial, _mlp], ids=["spatial", "mlp"])
def test_prep_gen_names_each_build(make):
    """tables of device pointers (ResNet._chain_cache) are keyed on _prep_gen: a rebuild must change it"""
    m = make()
    _prep(m)
    g0 = m._prep_gen
    _prep(m)
    assert m._prep_gen == g0
    _edit_mul(m, next(m.parameters()))
    _prep(m)
    assert m._prep_gen != g0


def test_prep_key_covers_buffers_and_sub_modules():
    """The key is every parameter AND buffer of the module's own sub-tree: BatchNorm statistics (BN re-estimation), the maskers a block owns.
    (The preparations of these modules need the device library; the key mechanics do not.)"""
    from laudnet_amd.laud_resnet import Bottleneck, Masker_channel_conv_linear
    mk = Masker_channel_conv_linear(32, 8).eval()
    blk = Bottleneck(32, 8, dyn_mode="channel", channel_masker="MLP", channel_dyn_granularity=2, output_size=14).eval()
    sites = [(mk, mk.conv[1].running_var), (mk, mk.conv[1].running_mean), (mk, mk.linear.bias),
             (blk, blk.bn2.running_mean), (blk, blk.bn3.running_var), (blk, blk.conv2.weight), (blk, blk.masker_channel.conv[2].weight)]
    for m, t in sites:
        m._cache_store(("prepared",))
        assert m._cache_valid()
        with torch.no_grad():
            t.mul_(4.0) if t.dim() else t.add_(1)
        assert not m._cache_valid(), f"{type(m).__name__}: an edit of a {tuple(t.shape)} source tensor went unnoticed"


# ---- the two documented blind spots: negative controls (these are the assertions above, failing)
@pytest.mark.parametrize("make", [_spatial, _mlp], ids=["spatial", "mlp"])
def test_control_an_edit_through_data_is_not_noticed(make):
    """`p.data` is a detached alias with a version counter of its own.  On a float64 module, where the float32 preparation is a real copy,
    the prepared values are then the OLD ones (on a float32 module some prepared tensors alias their parameter and follow it anyway: there
    only the validity is asserted)."""
    m = make()
    prep = _assert_prep(m, "float32")
    next(m.parameters()).data.mul_(2)
    assert m._cache_valid() and all(a is b for a, b in zip(_prep(m), prep)), "float32: the documented blind spot has closed -- update _PrepCache's docstring"
    m = make().double()
    _assert_prep(m, "float64")
    old = _expected(m)
    stale = [t.clone() for t in _prep(m)]
    for p in m.parameters():
        p.data.mul_(2)
    assert m._cache_valid(), "the documented blind spot has closed -- update _PrepCache's docstring"
    for got, kept, was, now in zip(_prep(m), stale, old, _expected(m)):
        assert torch.equal(got, kept) and torch.equal(got.double(), was.float().double()) and not torch.equal(got.double(), now.float().double())
    m.invalidate()
    assert not m._cache_valid()
    _assert_prep(m, "after invalidate()")


@pytest.mark.parametrize("make", [_spatial, _mlp], ids=["spatial", "mlp"])
def test_control_a_replaced_parameter_object_is_not_noticed(make):
    m = make()
    _assert_prep(m, "first preparation")
    old = _expected(m)
    lin = m.conv if hasattr(m, "_wb") else m.conv[2]
    lin.weight = nn.Parameter(seeded_randn(tuple(lin.weight.shape), 61))
    assert m._cache_valid(), "the documented blind spot has closed -- update _PrepCache's docstring"
    now = _expected(m)
    assert any(not torch.equal(a, b) for a, b in zip(old, now))
    for got, was in zip(_prep(m), old):
        assert torch.equal(got.double(), was), "the stale preparation holds the replaced parameter's values"
    m.invalidate()
    assert not m._cache_valid()
    _assert_prep(m, "after invalidate()")
