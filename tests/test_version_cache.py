"""ops.VersionCache on CPU tensors (no GPU): when an entry is served and when it is rebuilt, what a graph capture does to it (the capture
is mocked as in test_graphed_forward_recaptures_when_a_guard_moved), and that ops.invalidate_caches() reaches every cache."""
import gc
import types
import weakref

import torch

from dir_amd import dense, ops


class _Build:
    """build() for VersionCache.get: counts its calls, returns a new tensor each time."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return torch.zeros(2)


def test_entry_is_served_per_version_of_the_watched_tensors():
    cache = ops.VersionCache("t", limit=8)
    w = torch.nn.Parameter(torch.ones(4))
    build = _Build()
    a = cache.get("k", (w,), build, extra=(4,))
    assert cache.get("k", (w,), build, extra=(4,)) is a and build.calls == 1           # a repeated call: the same object, one build
    assert cache in ops.version_caches() and len(cache) == 1 and cache.values()[0][0] is a

    def rebuilt(watched=None, extra=(4,)):
        n, got = build.calls, cache.get("k", (w,) if watched is None else watched, build, extra=extra)
        again = cache.get("k", (w,) if watched is None else watched, build, extra=extra)
        return build.calls == n + 1 and again is got and len(cache) == 1

    with torch.no_grad():
        w.mul_(2.0)                                                                    # an in-place op
    assert rebuilt()
    w.data.mul_(2.0)
    ops.mark_written(w)                                                                # a raw write reported as the fused updaters do
    assert rebuilt()
    ops.invalidate_caches()
    assert len(cache) == 0 and rebuilt()
    assert rebuilt(extra=(5,))                                                         # a changed extra
    other = torch.nn.Parameter(torch.ones(4))                                          # another tensor object under the same key
    torch._C._autograd._unsafe_set_version_counter([other], [w._version])              # (at the same version: identity decides)
    assert rebuilt(watched=(other,))
    assert rebuilt()                                                                   # ... and back
    v = w._version
    del w
    gc.collect()
    w = torch.nn.Parameter(torch.ones(4))                                              # the watched tensor collected, a new one under the key
    torch._C._autograd._unsafe_set_version_counter([w], [v])                           # (at the dead one's version: identity decides)
    n = build.calls
    cache.get("k", (w,), build, extra=(4,))
    assert build.calls == n + 1


def test_inference_tensor_is_built_per_call():
    cache = ops.VersionCache("t", limit=8)
    with torch.inference_mode():
        w = torch.ones(4)
    normal = torch.ones(4)
    build = _Build()
    a, b = cache.get("k", (normal, w), build), cache.get("k", (normal, w), build)
    assert build.calls == 2 and a is not b and len(cache) == 0


def test_limit_clears_the_cache():
    cache = ops.VersionCache("t", limit=4)
    ws = [torch.ones(1) for _ in range(cache.limit + 2)]
    for i, w in enumerate(ws):
        cache.get(i, (w,), _Build())
        assert len(cache) <= cache.limit + 1
    assert len(cache) == 1                                                             # the last store found limit + 1 entries: cleared


def test_cache_keeps_no_watched_tensor_alive():
    cache = ops.VersionCache("t", limit=8)
    w = torch.nn.Parameter(torch.ones(4))
    cache.get("k", (w,), _Build())
    ref = weakref.ref(w)
    del w
    gc.collect()
    assert ref() is None and len(cache) == 1
    cache.clear()
    assert len(cache) == 0


def test_capture_rules(monkeypatch):
    state = {"capturing": False}
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: state["capturing"])
    cache = ops.VersionCache("t", limit=8)
    w, u = torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.ones(4))
    build = _Build()
    entry = cache.get("w", (w,), build)
    with ops.capture_hold() as hold:                                                   # a default capture: nothing read, nothing stored
        state["capturing"] = True
        got, new = cache.get("w", (w,), build), cache.get("u", (u,), build)
        state["capturing"] = False
    assert build.calls == 3 and got is not entry and new is not entry
    assert len(cache) == 1 and cache.values()[0][0] is entry and hold.keep == []
    with ops.frozen_weights() as hold:
        state["capturing"] = True
        got, new = cache.get("w", (w,), build), cache.get("u", (u,), build)            # a valid entry is served and held; a miss is built, not stored
        state["capturing"] = False
    assert build.calls == 4 and got is entry and new is not entry
    assert len(cache) == 1 and len(hold.keep) == 1 and hold.keep[0] is entry
    assert cache.get("w", (w,), build) is entry and build.calls == 4                   # outside: as before
    assert ops._HOLDS == [] and not ops._FROZEN_WEIGHTS[0]


def test_invalidate_caches_reaches_the_padded_weight_copies():
    w = torch.nn.Parameter(torch.ones(16, 48))
    p = dense._packed_cached(w)
    assert dense._packed_cached(w) is p and torch.equal(p, w.detach())
    w.data.mul_(2)                                                                     # bumps no version counter
    ops.invalidate_caches()
    p2 = dense._packed_cached(w)
    assert p2 is not p and torch.equal(p2, torch.full((16, 48), 2.0))
    q = dense._packed_cached(w, 4)                                                     # the zero-padded form: an entry of its own
    assert q.shape == (16, 52) and torch.equal(q[:, :48], p2) and not q[:, 48:].any() and dense._packed_cached(w, 4) is q


def _bn4():
    return types.SimpleNamespace(moving_mean=torch.zeros(4), moving_variance=torch.ones(4), beta=torch.zeros(4), gamma=None, eps=0.0)


def test_invalidate_caches_reaches_the_folded_batch_norms():
    bn = _bn4()
    scale, shift = dense._bn_affine(bn)
    assert dense._bn_affine(bn)[1] is shift and torch.equal(shift, torch.zeros(4)) and torch.equal(scale, torch.ones(4))
    bn.moving_mean.data.add_(1.0)                                                      # bumps no version counter
    ops.invalidate_caches()
    assert torch.equal(dense._bn_affine(bn)[1], torch.full((4,), -1.0))


def test_packed_weight_and_batch_norm_take_inference_tensors():
    with torch.inference_mode():
        w = torch.ones(16, 48)
        bn = _bn4()
    n_pack, n_bn = len(dense._PACK_CACHE), len(dense._BN_CACHE)
    p, p2 = dense._packed_cached(w), dense._packed_cached(w)
    assert p is not p2 and torch.equal(p, w) and torch.equal(p2, w) and len(dense._PACK_CACHE) == n_pack
    a, a2 = dense._bn_affine(bn), dense._bn_affine(bn)
    assert a[0] is not a2[0] and torch.equal(a[0], torch.ones(4)) and torch.equal(a[1], torch.zeros(4)) and len(dense._BN_CACHE) == n_bn


def test_invalidate_caches_moves_deepfm_pack_signature():
    from dir_amd import feature_column as fc
    from dir_amd.deepfm import DeepFM
    cats = [fc.categorical_column_with_identity("C%d" % i, v) for i, v in enumerate((7, 5, 11))]
    model = DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, 4) for c in cats], dnn_hidden_units=[16],
                   fm_embedding_size=4)
    sig = model._pack_signature()
    assert model._pack_signature() == sig
    ops.invalidate_caches()
    assert model._pack_signature() != sig
