"""_cache.py -- what is derived from a weight and remembered per version of it (packed images, padded copies, folded batch norms), and
how a HIP graph capture treats it.  ops re-exports every public name here.

A VersionCache entry stands for the tensors it was built from: it is served while they are the same objects at the same
tensor._version (in-place torch ops bump it; the fused updaters report their raw writes through ops.mark_written) and no
invalidate_caches() ran.  A graph keeps raw pointers only, so under a capture:
  default (capture_hold)  nothing is read or stored -- the pack kernels become part of the graph and read the weights as they are at
                          replay time;
  frozen_weights          valid entries are served and kept alive in the hold for the graph's lifetime; a miss is built inside the
                          graph and not stored (its memory belongs to the graph's pool).
"""
import operator
import weakref

import torch

_CACHE_GEN = [0]                 # bumped by invalidate_caches(): everything remembered before it is stale
_FROZEN_WEIGHTS = [False]
_HOLDS = []                      # the keep-alive lists of the captures in progress (capture_hold / frozen_weights), innermost last
_VERSION = operator.attrgetter("_version")
_CACHES = weakref.WeakSet()      # every VersionCache
also_cleared = []                # dicts outside the protocol that invalidate_caches() empties too (ops._WEIGHT_ABSMAX)


class capture_hold:
    """with ops.capture_hold() as hold: ... capture ...  -- what a graph captured inside reads through a cache.  A graph keeps raw pointers
    only: a cache entry it read may be dropped afterwards (an eager call at a new weight version replaces it, invalidate_caches() and the
    caches' size limits clear it) and the allocator may hand its block out again.  So every cache hit served while a stream is capturing
    appends what it returned to `keep` (tensors; a TableSet / PackedTables object) -- the owner of the graph stores the hold for the
    graph's lifetime -- and a cache that is NOT bypassed under a default capture (DeepFM's packed serving rows: a copy of the tables)
    records the tensors its entry was built from in `guards`: moved() is True once one of them was modified in place or invalidate_caches()
    ran, and the owner captures again (GraphedForward).  serving.GraphedForward and CapturedStep open one around their capture."""

    def __init__(self):
        self.keep, self._guard_ts, self._guard_ids = [], [], set()
        self._guard_vs, self._gen = [], _CACHE_GEN[0]

    def __enter__(self):
        _HOLDS.append(self)
        return self

    def __exit__(self, *exc):
        _HOLDS.remove(self)
        return False

    def guard(self, tensors):
        for t in tensors:
            if id(t) not in self._guard_ids:
                self._guard_ids.add(id(t))
                self._guard_ts.append(t)
                self._guard_vs.append(t._version)

    @property
    def guarded(self):
        return bool(self._guard_ts)

    def moved(self):
        """Whether a guarded tensor was modified in place (tensor._version) or invalidate_caches() ran since the capture."""
        return self._gen != _CACHE_GEN[0] or list(map(_VERSION, self._guard_ts)) != self._guard_vs


def held(obj, guards=()):
    """A cache hands `obj` to its caller: while a stream is capturing inside a capture_hold / frozen_weights, the hold keeps it alive (and
    records `guards`, see capture_hold).  Returns obj.  Outside a capture: nothing (one list test)."""
    if _HOLDS and torch.cuda.is_current_stream_capturing():
        h = _HOLDS[-1]
        h.keep.append(obj)
        if guards:
            h.guard(guards)
    return obj


def capture_guard(tensors):
    """A decision taken from the values of `tensors` now (a measured magnitude that picks a kernel's split) is baked into the graph being
    captured: the open hold records them as guards (capture_hold.moved)."""
    if _HOLDS and torch.cuda.is_current_stream_capturing():
        _HOLDS[-1].guard(tensors)


class frozen_weights(capture_hold):
    """with ops.frozen_weights() as hold: ... capture ...  -- a capture taken inside takes the VALID per-version cache entries (weight images,
    packed weights, folded batch norms: built by an earlier eager call on the same versions) instead of re-packing inside the graph.  For
    SERVING graphs whose weights do not change between replays: a one-launch DeepFM forward at 1 024-4 096 rows carries three pack launches
    otherwise (15-20 us of ~70).  The price: a replay after an in-place weight update still runs the images of capture time -- capture again
    after loading new weights.  What the graph reads stays valid: every entry it took is in `hold.keep` (capture_hold), which the owner of the
    graph stores, so an eager call at new weights, invalidate_caches() or a cache's size limit cannot free it under the graph.
    serving.GraphedForward(..., frozen_weights=True) uses it."""

    def __enter__(self):
        self._old = _FROZEN_WEIGHTS[0]
        _FROZEN_WEIGHTS[0] = True
        return super().__enter__()

    def __exit__(self, *exc):
        _FROZEN_WEIGHTS[0] = self._old
        return super().__exit__(*exc)


def capture_bypasses_caches(t=None):
    """True while the current stream is capturing and the per-version caches must not be read (the default rule; see frozen_weights).
    (The query needs a device: a CPU tensor `t` outside every hold is under no capture.)"""
    return bool((t is None or t.is_cuda or _HOLDS) and torch.cuda.is_current_stream_capturing() and not _FROZEN_WEIGHTS[0])


class VersionCache:
    """key -> a value built from the tensors `watched`, served per version of them (the module docstring has the rules).  `limit`: past
    this many entries the next store clears the cache first.  No strong reference to a watched tensor is kept."""

    def __init__(self, name, limit):
        self.name, self.limit, self._entries = name, limit, {}
        _CACHES.add(self)

    def get(self, key, watched, build, extra=()):
        """key: hashable, the entry's slot.  watched: the LONG-LIVED tensors whose identity and versions stand for the entry (a module's
        nn.Parameters, not their `.data` views: those are new objects on every call).  extra: what else must be unchanged, compared with == (shapes, strides,
        data_ptrs, eps).  build() makes the value."""
        capturing = (watched[0].is_cuda or _HOLDS) and torch.cuda.is_current_stream_capturing()      # (as capture_bypasses_caches, inline: every
        if capturing and not _FROZEN_WEIGHTS[0]:                                                     # eager forward comes through here)
            return build()
        hit = self._entries.get(key)
        if hit is not None and hit[2] == extra and hit[3] == _CACHE_GEN[0] and len(hit[0]) == len(watched):
            for t, ref, version in zip(watched, hit[0], hit[1]):       # (the same object first: only a stored tensor's _version is read)
                if ref() is not t or t._version != version:
                    break
            else:
                return held(hit[4]) if _HOLDS else hit[4]
        value = build()
        if not capturing and not any(t.is_inference() for t in watched):       # an inference tensor has no version counter to follow
            if len(self._entries) > self.limit:
                self._entries.clear()
            self._entries[key] = ([weakref.ref(t) for t in watched], [t._version for t in watched], extra, _CACHE_GEN[0], value)
        return value

    def values(self):
        """The cached values, each as the tuple of its parts -- an image tensor as a 1-tuple (for tests and tools: code that walks an
        item for its tensors must never be handed a bare tensor, which iterates element by element)."""
        return [e[4] if isinstance(e[4], tuple) else (e[4],) for e in self._entries.values()]

    def __len__(self):
        return len(self._entries)

    def clear(self):
        self._entries.clear()


def version_caches():
    """Every VersionCache alive (for tests and tools)."""
    return list(_CACHES)


def invalidate_caches():
    """Drop everything remembered per tensor version: every VersionCache entry, the magnitude measurements, DeepFM's packed serving rows
    (rebuilt on the next forward) -- and graphs captured under a capture_hold capture again.  The caches follow tensor._version, which
    in-place torch ops bump; a write through `param.data`, a raw-pointer kernel or a checkpoint loader that copies into storage directly
    does not -- call this after such a write (checkpoint.load_* do)."""
    for c in list(_CACHES) + also_cleared:
        c.clear()
    _CACHE_GEN[0] += 1


# ---- raw writes: what the fused updaters do to the version counters ---------------------------------------------------------------
_HIP_BUMPS = None                # version-counter owner (a view's base) -> how many of its version bumps mark_written made


def _vc_owner(t):
    return t._base if t._base is not None else t


def hip_bumps(t):
    """How many of tensor t's version bumps came from mark_written (a fused updater's step), not from torch ops: the magnitude caches
    (TableSet.absmax / weight_absmax with every > 1) tolerate only those."""
    return 0 if _HIP_BUMPS is None else _HIP_BUMPS.get(_vc_owner(t), 0)


def mark_written(*tensors):
    """A raw-pointer kernel has just written these tensors in place: bump their autograd version counters, as an in-place torch op would
    have.  Everything cached per weight version (DeepFM's packed serving rows and every VersionCache: ops.version_caches()) keys on
    tensor._version, so an eval -> train -> eval loop in one process (the reference's train_and_evaluate) rebuilds them after a HIP
    optimiser step.  Views share their base's counter."""
    global _HIP_BUMPS
    ts = [t for t in tensors if isinstance(t, torch.Tensor)]
    if ts:
        torch._C._autograd._unsafe_set_version_counter(ts, [t._version + 1 for t in ts])
        if _HIP_BUMPS is None:
            from torch.utils.weak import WeakIdKeyDictionary
            _HIP_BUMPS = WeakIdKeyDictionary()
        seen = set()
        for t in ts:
            o = _vc_owner(t)
            if id(o) not in seen:
                seen.add(id(o))
                _HIP_BUMPS[o] = _HIP_BUMPS.get(o, 0) + 1
