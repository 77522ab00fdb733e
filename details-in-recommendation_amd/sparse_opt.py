"""sparse_opt.py -- the fused sparse optimisers over a TableSet: SparseAdagrad, SparseAdam, SparseFtrl (ops re-exports them, and the
models and shard.py use the ops. names).  Each entry is a thin call through the C ABI (include/dir_hip.h: dir_sparse_*) on torch's
current HIP stream; what the entries share -- the row-base prefix, the sort area, the argument checks, the reuse of another update's
sort -- lives in _SortedOpt."""
import collections
import ctypes

import torch

from . import _lib
from ._abi import _stream, _dev, _ptr, _onehot_strides
from ._cache import mark_written


class _SortedShare:
    """Two sorted sparse updates of one training step that see the same (row, entry) pairs -- DeepFM's Adagrad on the embedding tables
    and FTRL on the linear columns of the same categorical columns (deepFM.py:58,61) -- sort once: whichever runs first in backward()
    leaves a token (the id tensor's identity and version, its layout, the stream) and its workspace, the other takes the sorted pairs
    from it (include/dir_hip.h: dir_sparse_*_sorted_*_from_f32).  A token is used at most once and only by the other optimiser."""

    def __init__(self):
        self.token = None
        self.owner = None
        self.ws = None
        self.ws_tensor = None
        self.hits = 0                       # sorts saved so far

    @staticmethod
    def _token(ids, B, sb, sf):
        return (ids.data_ptr(), ids._version, B, sb, sf, torch.cuda.current_stream(ids.device).cuda_stream)

    def take(self, who, ids, B, sb, sf):
        """-> the other optimiser's workspace pointer if it sorted exactly these entries last, else None."""
        if self.token is not None and self.owner is not who and self.token == self._token(ids, B, sb, sf) \
                and self.owner._ws is self.ws_tensor:               # (the owner's workspace has not been reallocated since)
            ws = self.ws
            self.token = None
            self.hits += 1
            return ws
        return None

    def leave(self, who, ids, B, sb, sf, ws):
        self.token, self.owner, self.ws, self.ws_tensor = self._token(ids, B, sb, sf), who, ws, who._ws


def share_sorted_entries(a, b):
    """Let two sorted sparse optimisers over table sets with the same vocabularies share one sort per step (see _SortedShare).
    -> True if they were linked."""
    if list(a.ts.vocab) != list(b.ts.vocab) or a.ts.F != b.ts.F or getattr(a, "method", "sorted") != "sorted":
        return False
    if a.ts.shared or b.ts.shared:          # a sharing set's keys run over its distinct tables: not the other set's keys
        return False
    a._share = b._share = _SortedShare()
    return True


def _aligned(buf):
    """-> (the first 256-byte aligned address inside the uint8 tensor buf, the bytes behind it)"""
    p = buf.data_ptr()
    off = (-p) % 256
    return ctypes.c_void_p(p + off), buf.numel() - off


class _SortedOpt:
    """What the three optimisers share.  ts: the TableSet; row_base [F] device int64 / total_rows: the tables' rows as one key range;
    _ws: the sort area (a linked optimiser -- _share, sorted_by= -- reads the sorted pairs out of it); _slots: the optimiser's own
    state tensors, whose version counters move with the tables'."""

    def __init__(self, tables):
        from .ops import _as_tableset          # (ops imports this module: the name is taken where it is used, once per optimiser)
        self.ts = _as_tableset(tables)
        # the key space runs over the DISTINCT tables (ts.row_base [T]); without sharing that is one table per slot
        self.total_rows = self.ts.total_rows
        self.row_base = self.ts.row_base
        self._slots = []
        self._ws = None
        self._share = None

    def _refuse_shared(self, entry):
        """Only the one-hot steps of SparseAdagrad and SparseAdam know the slot -> table map: everything else refuses a set that shares
        tables."""
        if self.ts.shared:
            raise ValueError("%s does not cover tables shared between slots (slots %s read one table)"
                             % (entry, self.ts.slots_of(next(t for t in range(self.ts.T) if len(self.ts.slots_of(t)) > 1))))

    def _ptr_array(self, tensors):
        """The [F] device array of base pointers the kernels read table f's slot through."""
        return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64, device=self.ts.device)

    def _written(self):
        """The update kernels write the tables and slots through raw pointers: version counters bumped here (ops.mark_written), once per
        call that launched, after the launch returned OK."""
        self.ts.written(*self._slots)

    # ---- the sort area -------------------------------------------------------------------------------------------------------------
    def _sort_need(self, entry, query, *dims):
        """-> the bytes query(*dims, total_rows) asks for (include/dir_hip.h: dir_sparse_*_workspace_bytes; 0 says unsupported)."""
        need = int(query(*dims, self.total_rows))
        if need <= 0:
            raise _lib.DirError(-4, "%s: unsupported size %s over %d rows (include/dir_hip.h: %s)" % (entry, dims, self.total_rows, query.__name__))
        return need

    def _sort_area(self, entry, query, *dims, buf="_ws"):
        """The buffer self.<buf> grown to what the query asks for (never shrunk) -> (its 256-byte aligned pointer, the bytes asked for,
        the bytes behind the pointer)."""
        need = self._sort_need(entry, query, *dims)
        area = getattr(self, buf)
        if area is None or area.numel() < need + 256:
            area = torch.empty(need + 256, dtype=torch.uint8, device=self.ts.device)
            setattr(self, buf, area)
        ws, behind = _aligned(area)
        return ws, need, behind

    def _sorted_by(self, entry, other):
        """sorted_by=other: -> the sort area of the optimiser that has JUST sorted the same entries on this stream (None: sort here)."""
        if other is None:
            return None
        if other.total_rows != self.total_rows or list(other.ts.vocab) != list(self.ts.vocab) or other._ws is None:
            raise ValueError("%s: sorted_by must have just sorted the same entries over the same local vocabularies" % entry)
        return _aligned(other._ws)[0]

    def _take_sort(self, ids, B, sb, sf):
        return self._share.take(self, ids, B, sb, sf) if self._share is not None else None

    def _leave_sort(self, ids, B, sb, sf, ws):
        if self._share is not None:
            self._share.leave(self, ids, B, sb, sf, ws)

    # ---- argument checks -----------------------------------------------------------------------------------------------------------
    def _check_onehot(self, ids, grad, widths, grad_optional=False):
        """ids [B, F] int64 (any strides), grad [B, w] fp32 with unit inner stride, w one of widths -> (B, stride_b, stride_f)"""
        _dev(ids, torch.int64, "ids")
        B, sb, sf = _onehot_strides(ids, self.ts.F)
        if grad is not None or not grad_optional:
            _dev(grad, torch.float32, "grad")
            if grad.dim() != 2 or grad.shape[0] != B or grad.shape[1] not in widths or grad.stride(1) != 1:
                raise ValueError("grad must be %s with unit inner stride" % ("[B, F*K]" if len(widths) == 1 else "[B, F*K] or [B, K]"))
        return B, sb, sf

    def _check_payload(self, payload, grad, width, exact=True):
        """payload [n] int64, grad fp32 [n, width] in payload order (exact=False: any shape of n * width elements), both contiguous -> n"""
        _dev(payload, torch.int64, "payload")
        _dev(grad, torch.float32, "grad")
        n = payload.numel()
        ok = grad.shape == (n, width) if exact else grad.numel() == n * width
        if not ok or not grad.is_contiguous() or not payload.is_contiguous():
            raise ValueError("grad must be a contiguous %s tensor matching the payload" % ("[n, %d]" % width if exact or width > 1 else "[n]"))
        return n

    def _check_bags(self, entry, recv, P, cap_e, cap_b, grad, width, slot_mn=None):
        """recv: P bag slabs of (cap_e + 1) 16-byte records, grad fp32 [P*cap_b, width] (width None: P*cap_b floats), slot_mn [F] fp32 or
        None, all contiguous."""
        _dev(recv, torch.int64, "recv")
        _dev(grad, torch.float32, "grad")
        ok = grad.numel() == P * cap_b if width is None else grad.shape == (P * cap_b, width)
        if recv.numel() < P * (cap_e + 1) * 2 or not ok or not grad.is_contiguous() or not recv.is_contiguous():
            raise ValueError("%s: recv [P*(cap_e+1)*2] int64, grad a contiguous %s tensor" % (entry, "[P*cap_b]" if width is None else "[P*cap_b, K]"))
        if slot_mn is not None:
            _dev(slot_mn, torch.float32, "slot_mn")
            if slot_mn.numel() != self.ts.F or not slot_mn.is_contiguous():
                raise ValueError("%s: slot_mn must be a contiguous [F] float32 tensor" % entry)


class SparseAdagrad(_SortedOpt):
    """Fused sparse Adagrad over a TableSet.  Holds the accumulators ([TF-upstream] initial_accumulator_value = 0.1).
    method "sorted" (default; include/dir_hip.h: dir_sparse_adagrad_sorted_f32): radix sort of (row, entry) pairs +
    per-tile segmented reduce -- skew-proof and bitwise reproducible.  method "chains" (dir_sparse_adagrad_f32): per-row
    chains built with integer atomics -- a little faster on near-unique ids, serialises on hot rows.
    A TableSet.train_rows set brings its accumulators with it (packed [embedding | accumulator] rows: one read and one write
    per touched row; dir_sparse_adagrad_sorted_rows_f32); step_fm folds the FM backward into the update on either layout."""

    def __init__(self, tables, lr, initial_accumulator_value=0.1, method="sorted"):
        if method not in ("sorted", "chains"):
            raise ValueError("method must be 'sorted' or 'chains'")
        super().__init__(tables)
        self.lr = float(lr)
        self.method = method
        if self.ts.shared and method != "sorted":
            # the chains are built per (slot, id): a shared row would get one chain -- and one step -- per slot
            raise ValueError("method='chains' does not cover tables shared between slots: use the sorted method")
        if self.ts.accums is not None:           # packed training rows: the accumulators live beside the embeddings
            if method != "sorted":
                raise ValueError("packed training rows are updated by the sorted method")
            self.accums = self.ts.accums
        else:
            # one accumulator per TABLE; .accums stays indexed by slot (the slots of a shared table hold the same tensor)
            per_table = [torch.full_like(t, initial_accumulator_value) for t in self.ts.distinct]
            self.accums = [per_table[t] for t in self.ts.slot_table]
        self._slots = [] if getattr(self.ts, "arena", None) is not None else self.accums      # (one arena: its counter covers the accumulators)
        self.acc_ptrs = self._ptr_array(self.accums)
        self.head = torch.full((self.total_rows,), -1, dtype=torch.int32, device=self.ts.device) if method == "chains" else None
        self._next = None

    def attach(self):
        """Consume the gather's row gradients directly in backward (autograd.GatherFm): loss.backward() then
        performs the embedding update itself; the tables get no .grad."""
        self.ts.grad_sink = self.step
        if self.method == "sorted":
            self.ts.fm_sink = self.step_fm
        return self

    def _rows_update(self, lib, ids, B, sb, sf, grad, fm_g, fm_sum):
        """dir_sparse_adagrad_sorted_rows_f32, or its _from form when the linked optimiser has just sorted the same entries."""
        ts = self.ts
        ws, need, _ = self._sort_area("SparseAdagrad.step", lib.dir_sparse_adagrad_sorted_workspace_bytes, B, ts.F, ts.K)
        if ts.shared:                            # (never linked to another optimiser's sort: share_sorted_entries refuses a sharing set)
            _lib.check(lib.dir_sparse_adagrad_sorted_rows_shared_f32(
                _ptr(ts._ptrs), _ptr(self.acc_ptrs), ts.ld, ts.F, ts.K, _ptr(ids), sb, sf, _ptr(grad), grad.stride(0) if grad is not None else 0,
                _ptr(fm_g), _ptr(fm_sum), self.lr, B, _ptr(self.row_base), self.total_rows, _ptr(ts.slot_table_dev), ts.T, ws, need, _stream()))
            self._written()
            return
        src = self._take_sort(ids, B, sb, sf)
        args = (_ptr(ts._ptrs), _ptr(self.acc_ptrs), ts.ld, ts.F, ts.K, _ptr(ids), sb, sf, _ptr(grad), grad.stride(0) if grad is not None else 0,
                _ptr(fm_g), _ptr(fm_sum), self.lr, B, _ptr(self.row_base), self.total_rows, ws, need)
        if src is not None:
            _lib.check(lib.dir_sparse_adagrad_sorted_rows_from_f32(*args, src, _stream()))
        else:
            _lib.check(lib.dir_sparse_adagrad_sorted_rows_f32(*args, _stream()))
            self._leave_sort(ids, B, sb, sf, ws)
        self._written()

    def step_fm(self, ids, grad, fm_g, fm_sum):
        """The update with the FM backward folded in (include/dir_hip.h: dir_sparse_adagrad_sorted_rows_f32): entry (b, f)'s
        gradient is (fm_sum[b] - row) * fm_g[b] + grad[b, f].  grad [B, F*K] or None, fm_g [B] / [B, 1], fm_sum [B, K] from
        gather_fm(..., fsum=).  Tables bit-identical to fm_logit_backward(add_in=grad) followed by step()."""
        ts = self.ts
        B, sb, sf = self._check_onehot(ids, grad, (ts.F * ts.K,), grad_optional=True)
        _dev(fm_g, torch.float32, "fm_g")
        _dev(fm_sum, torch.float32, "fm_sum")
        if fm_g.numel() != B or not fm_g.is_contiguous() or fm_sum.shape != (B, ts.K) or not fm_sum.is_contiguous():
            raise ValueError("fm_g must be a contiguous [B] / [B, 1] tensor and fm_sum a contiguous [B, K] one")
        if B == 0:
            return
        self._rows_update(_lib.load(), ids, B, sb, sf, grad, fm_g, fm_sum)

    def step(self, ids, grad):
        """ids [B, F] int64 (any strides), grad [B, F*K] fp32: d loss / d gathered rows."""
        ts = self.ts
        B, sb, sf = self._check_onehot(ids, grad, (ts.F * ts.K,))
        if B == 0:
            return
        lib = _lib.load()
        if ts.ld != ts.K or (self._share is not None and self.method == "sorted"):
            self._rows_update(lib, ids, B, sb, sf, grad, None, None)
            return
        if ts.shared:
            ws, need, _ = self._sort_area("SparseAdagrad.step", lib.dir_sparse_adagrad_sorted_workspace_bytes, B, ts.F, ts.K)
            _lib.check(lib.dir_sparse_adagrad_sorted_shared_f32(_ptr(ts.ptrs), _ptr(self.acc_ptrs), ts.F, ts.K, _ptr(ids), sb, sf,
                                                                _ptr(grad), grad.stride(0), self.lr, B, _ptr(self.row_base),
                                                                self.total_rows, _ptr(ts.slot_table_dev), ts.T, ws, need, _stream()))
            self._written()
            return
        if self.method == "chains":
            if self._next is None or self._next.numel() < B * ts.F:
                self._next = torch.empty(B * ts.F, dtype=torch.int32, device=ts.device)
            _lib.check(lib.dir_sparse_adagrad_f32(_ptr(ts.ptrs), _ptr(self.acc_ptrs), ts.F, ts.K, _ptr(ids), sb, sf,
                                                  _ptr(grad), grad.stride(0), self.lr, B, _ptr(self.row_base),
                                                  self.total_rows, _ptr(self.head), _ptr(self._next), _stream()))
        else:
            ws, need, _ = self._sort_area("SparseAdagrad.step", lib.dir_sparse_adagrad_sorted_workspace_bytes, B, ts.F, ts.K)
            _lib.check(lib.dir_sparse_adagrad_sorted_f32(_ptr(ts.ptrs), _ptr(self.acc_ptrs), ts.F, ts.K, _ptr(ids), sb, sf,
                                                         _ptr(grad), grad.stride(0), self.lr, B, _ptr(self.row_base),
                                                         self.total_rows, ws, need, _stream()))
        self._written()

    def step_payload(self, payload, grad):
        """Owner side of a sharded backward (shard.ShardedTables): payload [n] int64 (local_row * F + slot, < 0 pruned) as
        received from all ranks, grad [n, K] in the same order (include/dir_hip.h: dir_sparse_adagrad_sorted_payload_f32)."""
        ts = self.ts
        self._refuse_shared("SparseAdagrad.step_payload")
        n = self._check_payload(payload, grad, ts.K)
        if n == 0:
            return
        lib = _lib.load()
        ws, need, _ = self._sort_area("SparseAdagrad.step_payload", lib.dir_sparse_adagrad_sorted_workspace_bytes, n, 1, ts.K)
        _lib.check(lib.dir_sparse_adagrad_sorted_payload_f32(_ptr(ts.ptrs), _ptr(self.acc_ptrs), ts.F, ts.K, _ptr(payload), n,
                                                             _ptr(grad), self.lr, _ptr(self.row_base), self.total_rows, ws, need,
                                                             _stream()))
        self._written()

    def step_bags(self, recv, P, cap_e, cap_b, grad_rows, slot_mn=None, mn=0.0):
        """Owner side of a sharded multi-hot backward (shard.ShardedTables.lookup_bags_train; include/dir_hip.h:
        dir_sparse_adagrad_sorted_bags_f32): recv = the P bag slabs of (cap_e + 1) 16-byte records the forward received, grad_rows
        [P*cap_b, K] = the gradients of the partial rows as received.  Entry (s, j) adds w * grad_rows[s*cap_b + ret] to its row; every
        touched row takes one Adagrad step with its summed gradient, through the slot's max_norm clip derivative (slot_mn [F] device
        fp32 or None + mn, as ops.slot_max_norms gives them) at its pre-update value."""
        ts = self.ts
        self._refuse_shared("SparseAdagrad.step_bags")
        if ts.ld != ts.K:
            raise ValueError("step_bags: plain [vocab, K] tables")
        self._check_bags("step_bags", recv, P, cap_e, cap_b, grad_rows, ts.K, slot_mn)
        if self.total_rows == 0:
            return
        lib = _lib.load()
        ws, need, _ = self._sort_area("SparseAdagrad.step_bags", lib.dir_sparse_adagrad_sorted_workspace_bytes, P * cap_e, 1, ts.K)
        _lib.check(lib.dir_sparse_adagrad_sorted_bags_f32(_ptr(ts.ptrs), _ptr(self.acc_ptrs), ts.F, ts.K, _ptr(recv), P, cap_e, cap_b,
                                                          _ptr(grad_rows), _ptr(slot_mn), float(mn), self.lr, _ptr(self.row_base),
                                                          self.total_rows, ws, need, _stream()))
        self._written()


# What a norm half leaves for the apply half: src (the payload / the slabs) at this version, sorted in this area on this stream;
# geometry: the slabs' (P, cap_e, cap_b), None for a payload.
_AdamSort = collections.namedtuple("_AdamSort", "src version area stream geometry")


class SparseAdam(_SortedOpt):
    """tf.train.AdamOptimizer on the embedding tables of a TableSet, in place, from the gather's row gradients (include/dir_hip.h:
    dir_sparse_adam_f32; the reference's train_op: DeepCrossNetwork.py:264-290, train.py:119-124).  [TF-upstream] semantics: every row of
    m, v and var moves every step (IndexedSlices gradients are zero outside the looked-up rows), each table's gradient is clipped on its
    own with tf.clip_by_norm(g, clip_norm) first.  Holds m and v (zeros, like the slots TF creates).  Set .lr_t before every step
    (lr * sqrt(1 - beta2^t) / (1 - beta1^t), t = global_step + 1); attach() makes loss.backward() perform the update.
    On the shards of row-sharded tables the same step runs in two halves, norm_payload / step_payload, around the ranks' sum of the norm
    shares (shard.ShardedTables.enable_training_adam); norm_bags / step_bags are the same halves over the bag records of a multi-hot
    lookup (lookup_bags_train), on the same marks, norm words and sort area: one-hot and bag steps may alternate.  sort_reuses counts
    the apply halves that ran on their norm half's sort; forget_sort() makes the next one sort for itself.
    Over a set that shares tables between slots (shared_embedding_columns) step() and step_table_grad() treat a shared table as the ONE
    variable it is (dir_sparse_adam_shared_f32): one m / v per table (.ms / .vs stay indexed by slot: the slots of a table hold the same
    tensor), one clip norm over the sum of all its slots' gradients, one step per row, one sweep per table.  Such a set is taken with
    shared=True only -- a TableSet shares by storage, whoever built it, and the step of a shared variable is not the per-slot step: the
    caller says that it means one --; without it the constructor refuses the set, as before.  The owner-side halves always refuse it."""

    def __init__(self, tables, beta1=0.9, beta2=0.999, eps=1e-8, clip_norm=0.0, shared=False):
        super().__init__(tables)
        ts = self.ts
        if not shared:
            self._refuse_shared("SparseAdam without shared=True")
        if ts.ld != ts.K:
            raise ValueError("SparseAdam: plain [vocab, K] tables")
        self.beta1, self.beta2, self.eps, self.clip_norm = float(beta1), float(beta2), float(eps), float(clip_norm)
        self.lr_t = 0.0
        # one m / v per TABLE; .ms / .vs stay indexed by slot (the slots of a shared table hold the same tensor)
        per_m, per_v = [torch.zeros_like(t) for t in ts.distinct], [torch.zeros_like(t) for t in ts.distinct]
        self.ms = [per_m[t] for t in ts.slot_table]
        self.vs = [per_v[t] for t in ts.slot_table]
        self._slots = per_m + per_v
        self.m_ptrs, self.v_ptrs = self._ptr_array(self.ms), self._ptr_array(self.vs)
        self._ws_B = -1                         # step()'s buffer (_ws) holds its marks: reallocated only when B grows
        self._pws, self._norm2, self._marks, self._sorted = None, None, None, None      # the halves' sort area, norm words, row marks and sort token
        self.steps = 0
        self.sort_reuses = 0

    @staticmethod
    def covers(ts):
        return ts.ld == ts.K and ts.F <= 64 and ts.K % 4 == 0 and 64 % (ts.K // 4) == 0 and sum(ts.vocab) < 0xffffffff

    def attach(self):
        self.ts.grad_sink = self.step
        return self

    def forget_sort(self):
        """Drop what the last norm half left: the next apply half runs its own key pass and sort."""
        self._sorted = None

    def step(self, ids, grad):
        """ids [B, F] int64 (any strides), grad [B, F*K] fp32 = d loss / d gathered rows: one Adam step of ALL rows of every table."""
        ts = self.ts
        B, sb, sf = self._check_onehot(ids, grad, (ts.F * ts.K,))
        lib = _lib.load()
        need = self._sort_need("SparseAdam.step", lib.dir_sparse_adam_workspace_bytes, B, ts.F, ts.K)
        first = 0
        if self._ws is None or self._ws_B < B:
            # the marks (behind the 1024 bytes of the norm words) must survive from step to step: the buffer is allocated once per batch size (grown,
            # never shrunk), zeroed by the first call
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=ts.device)
            self._ws_B = B
            first = 1
        ws, behind = _aligned(self._ws)
        args = (_ptr(ts.ptrs), _ptr(self.m_ptrs), _ptr(self.v_ptrs), ts.F, ts.K, _ptr(ids), sb, sf, _ptr(grad), grad.stride(0), self.lr_t,
                self.beta1, self.beta2, self.eps, self.clip_norm, B, _ptr(self.row_base), self.total_rows, ws, behind, first, _stream())
        if ts.shared:                           # keys, norm words, marks and the sweep over the distinct tables
            _lib.check(lib.dir_sparse_adam_shared_f32(*args, _ptr(ts.slot_table_dev), ts.T))
        else:
            _lib.check(lib.dir_sparse_adam_f32(*args))
        self._written()
        self.steps += 1

    # ---- the owner side of a sharded backward (shard.ShardedTables.enable_training_adam): the step in two halves -----------------
    # over a payload (norm_payload / step_payload) or over received bag records (norm_bags / step_bags); both forms on one sort area
    # (_pws: grows with the entries; the marks live apart), one set of marks and norm words.
    def _payload_area(self, entry, payload, grad):
        ts = self.ts
        n = self._check_payload(payload, grad, ts.K)
        lib = _lib.load()
        ws, _, behind = self._sort_area(entry, lib.dir_sparse_adam_payload_workspace_bytes, n, ts.F, ts.K, buf="_pws")
        return lib, n, ws, behind

    def _bags_area(self, entry, recv, P, cap_e, cap_b, grad_rows, slot_mn):
        ts = self.ts
        self._check_bags(entry, recv, P, cap_e, cap_b, grad_rows, ts.K, slot_mn)
        lib = _lib.load()
        ws, _, behind = self._sort_area(entry, lib.dir_sparse_adam_bags_workspace_bytes, P, cap_e, ts.F, ts.K, buf="_pws")
        return lib, ws, behind

    def _norm(self, src, geometry, launch):
        """A norm half: launch(norm words, stream) -> rc.  -> norm2 [2, F] device int64 with the carry taken; leaves the sort token."""
        if self._norm2 is None:
            self._norm2 = torch.zeros(_lib.ADAM_NORM_WORDS, dtype=torch.int64, device=self.ts.device)      # 64 low words, 64 high words
        stream = _stream()
        _lib.check(launch(_ptr(self._norm2), stream))
        # what the apply half may reuse: this tensor, unchanged, in this sort area, on this stream
        self._sorted = _AdamSort(src, src._version, self._pws, stream.value, geometry)
        words = self._norm2.view(2, 64)[:, :self.ts.F]
        return torch.stack([words[0] & 0xffffffff, words[1] + ((words[0] >> 32) & 0xffffffff)])

    def _apply(self, entry, src, geometry, sortable, norm2_global, launch):
        """An apply half: launch(marks, sorted, first_call, stream) -> rc.  sorted = 1 when the norm half's token names exactly this
        src (same object, same version), this sort area, this stream and this geometry -- and there is something to sort."""
        if (self.clip_norm > 0) != (norm2_global is not None):
            raise ValueError("%s: norm2_global goes with clip_norm > 0 (clip_norm=%g)" % (entry, self.clip_norm))
        if norm2_global is not None:
            _dev(norm2_global, torch.float64, "norm2_global")
            if norm2_global.numel() != self.ts.F or not norm2_global.is_contiguous():
                raise ValueError("norm2_global must be a contiguous [F] float64 tensor")
        first = 0
        if self._marks is None:
            self._marks = torch.empty(max(256, (self.total_rows + 255) // 256 * 256), dtype=torch.uint8, device=self.ts.device)
            first = 1
        stream = _stream()
        was, self._sorted = self._sorted, None
        reuse = 1 if (sortable and was is not None and was.src is src and was.version == src._version and was.area is self._pws
                      and was.stream == stream.value and was.geometry == geometry) else 0
        try:
            _lib.check(launch(_ptr(self._marks), reuse, first, stream))
        except _lib.DirError:
            self._marks = None         # a step that failed between its two passes may have left marks set: the next call zeroes them again
            raise
        self.sort_reuses += reuse
        self._written()
        self.steps += 1

    def norm_payload(self, payload, grad):
        """First half (include/dir_hip.h: dir_sparse_adam_payload_norm_f32): payload [n] int64 (local_row * F + slot, < 0 pruned) as
        received from all ranks, grad [n, K] in the same order; n == 0 is legal.  -> norm2 [2, F] device int64: THIS owner's share of
        every table's ||g||^2 as the kernel's two norm words with the carry taken -- row 0 the low word (the fraction in units of 2^-32,
        < 2^32), row 1 the high word (the integer part): share = high + low * 2^-32, exact for ||g|| < 2^31.  The payload stays sorted in
        the workspace for step_payload."""
        ts = self.ts
        self._refuse_shared("SparseAdam.norm_payload")
        lib, n, ws, behind = self._payload_area("SparseAdam.norm_payload", payload, grad)
        return self._norm(payload, None, lambda norm2, stream: lib.dir_sparse_adam_payload_norm_f32(
            ts.F, ts.K, _ptr(payload), n, _ptr(grad), _ptr(self.row_base), self.total_rows, norm2, ws, behind, stream))

    def step_payload(self, payload, grad, norm2_global=None):
        """Second half (dir_sparse_adam_payload_apply_f32): one Adam step of ALL local rows -- the touched ones from the payload, clipped
        with norm2_global [F] device float64 = every table's GLOBAL ||g||^2 (the owners' norm_payload shares summed over the ranks:
        high + low / 2^32; None exactly when clip_norm == 0), the others by the decay pass; n == 0 runs that pass alone.  The sort of a
        norm_payload call on the same payload just before is reused."""
        ts = self.ts
        self._refuse_shared("SparseAdam.step_payload")
        lib, n, ws, behind = self._payload_area("SparseAdam.step_payload", payload, grad)
        self._apply("step_payload", payload, None, n > 0, norm2_global, lambda marks, sorted_, first, stream: lib.dir_sparse_adam_payload_apply_f32(
            _ptr(ts.ptrs), _ptr(self.m_ptrs), _ptr(self.v_ptrs), ts.F, ts.K, _ptr(payload), n, _ptr(grad), self.lr_t, self.beta1, self.beta2,
            self.eps, self.clip_norm, _ptr(norm2_global), _ptr(self.row_base), self.total_rows, marks, ws, behind, sorted_, first, stream))

    def norm_bags(self, recv, P, cap_e, cap_b, grad_rows, slot_mn=None, mn=0.0):
        """First half over bag records (include/dir_hip.h: dir_sparse_adam_bags_norm_f32): recv = the P bag slabs of (cap_e + 1) 16-byte
        records the forward received, grad_rows [P*cap_b, K] = the gradients of the partial rows as received, slot_mn [F] device fp32 or
        None + mn as ops.slot_max_norms gives them.  A row's gradient is the sum of w * grad_rows[s*cap_b + ret] over all its entries,
        through the slot's max_norm clip derivative at the row's current value.  -> norm2 [2, F] device int64, as norm_payload.  The
        records stay sorted in the workspace for step_bags."""
        ts = self.ts
        self._refuse_shared("SparseAdam.norm_bags")
        lib, ws, behind = self._bags_area("norm_bags", recv, P, cap_e, cap_b, grad_rows, slot_mn)
        return self._norm(recv, (P, cap_e, cap_b), lambda norm2, stream: lib.dir_sparse_adam_bags_norm_f32(
            _ptr(ts.ptrs), ts.F, ts.K, _ptr(recv), P, cap_e, cap_b, _ptr(grad_rows), _ptr(slot_mn), float(mn), _ptr(self.row_base),
            self.total_rows, norm2, ws, behind, stream))

    def step_bags(self, recv, P, cap_e, cap_b, grad_rows, norm2_global=None, slot_mn=None, mn=0.0):
        """Second half over bag records (dir_sparse_adam_bags_apply_f32): one Adam step of ALL local rows -- the touched ones from their
        summed record gradients (through the max_norm clip derivative at the pre-update row), clipped with norm2_global [F] device
        float64 (None exactly when clip_norm == 0), the others by the decay pass; slabs without a live record run that pass alone.  The
        sort of a norm_bags call on the same slabs just before is reused."""
        ts = self.ts
        self._refuse_shared("SparseAdam.step_bags")
        lib, ws, behind = self._bags_area("step_bags", recv, P, cap_e, cap_b, grad_rows, slot_mn)
        self._apply("step_bags", recv, (P, cap_e, cap_b), True, norm2_global, lambda marks, sorted_, first, stream: lib.dir_sparse_adam_bags_apply_f32(
            _ptr(ts.ptrs), _ptr(self.m_ptrs), _ptr(self.v_ptrs), ts.F, ts.K, _ptr(recv), P, cap_e, cap_b, _ptr(grad_rows), _ptr(slot_mn),
            float(mn), self.lr_t, self.beta1, self.beta2, self.eps, self.clip_norm, _ptr(norm2_global), _ptr(self.row_base), self.total_rows,
            marks, ws, behind, sorted_, first, stream))

    def step_table_grad(self, f, grad):
        """Table f's step from a gradient that arrived as its .grad instead of through the sink -- multi-hot / weighted columns, whose
        backward (autograd.EmbeddingBag) returns sparse row gradients: the same tf.train.AdamOptimizer step of ALL rows (clip_by_norm on
        the table's gradient first) on this optimiser's m / v, with torch ops (not a hot path: the one-hot lookups take the HIP update).
        f is a SLOT.  A table shared between slots is one variable: autograd has summed every sharing column's contribution into the one
        parameter's .grad, and the table takes ONE step -- call this once per table (any one of its slots), not once per slot."""
        t, m, v = self.ts.tables[f], self.ms[f], self.vs[f]
        g = (grad.coalesce().to_dense() if grad.is_sparse else grad).to(torch.float32)
        if self.clip_norm > 0:
            g = g * (self.clip_norm / torch.clamp(torch.linalg.vector_norm(g), min=self.clip_norm))
        m.mul_(self.beta1).add_(g, alpha=1.0 - self.beta1)
        v.mul_(self.beta2).addcmul_(g, g, value=1.0 - self.beta2)
        t.addcdiv_(m, v.sqrt().add_(self.eps), value=-self.lr_t)
        owners = self.ts.owners                 # per slot, or each table's parameter once (InputLayer over shared columns)
        i = f if len(owners) == self.ts.F else self.ts.slot_table[f]
        mark_written(*owners[i:i + 1])

    def state_dict(self):
        """m and v of every DISTINCT table (a shared table's state once), in TableSet.distinct order, and the step count."""
        first = [self.ts.slots_of(t)[0] for t in range(self.ts.T)]
        return {"m": [self.ms[f].clone() for f in first], "v": [self.vs[f].clone() for f in first], "steps": self.steps}

    def load_state_dict(self, state):
        """Restore what state_dict() gave, in place (the kernels' pointer arrays stay valid)."""
        first = [self.ts.slots_of(t)[0] for t in range(self.ts.T)]
        if len(state["m"]) != len(first) or len(state["v"]) != len(first):
            raise ValueError("SparseAdam.load_state_dict: %d tables, state of %d" % (len(first), len(state["m"])))
        with torch.no_grad():
            for f, m, v in zip(first, state["m"], state["v"]):
                self.ms[f].copy_(m)
                self.vs[f].copy_(v)
        self.steps = int(state["steps"])
        mark_written(*self._slots)


class SparseFtrl(_SortedOpt):
    """Fused sparse FTRL-Proximal over a TableSet (include/dir_hip.h: dir_sparse_ftrl_sorted_f32; the reference's
    linear_optimizer='Ftrl', deepFM.py:58, with [TF-upstream] tf.train.FtrlOptimizer defaults: initial accumulator 0.1,
    learning_rate_power -0.5, l1 = l2 = 0).  step(ids, grad): grad is [B, F*K] (one gradient row per slot) or [B, K] (the same
    row for every slot: the linear term, whose d logit is shared by all columns)."""

    def __init__(self, tables, lr=0.2, initial_accumulator_value=0.1, l1=0.0, l2=0.0):
        super().__init__(tables)
        self._refuse_shared("SparseFtrl")
        self.lr, self.l1, self.l2 = float(lr), float(l1), float(l2)
        self.packed = getattr(self.ts, "linears", None) is not None      # TableSet.ftrl_rows: n and z live in the weights' rows
        if self.packed:
            self.accums, self.linears = self.ts.accums, self.ts.linears
        else:
            if self.ts.ld != self.ts.K:
                raise ValueError("SparseFtrl: tables with a row stride must be TableSet.ftrl_rows")
            self.accums = [torch.full_like(t, initial_accumulator_value) for t in self.ts.tables]
            self.linears = [torch.zeros_like(t) for t in self.ts.tables]
        self._slots = list(self.accums) + list(self.linears)
        self.acc_ptrs, self.lin_ptrs = self._ptr_array(self.accums), self._ptr_array(self.linears)

    def attach(self):
        """Consume the linear term's gradient directly in backward (autograd.LinearLogit)."""
        self.ts.grad_sink = self.step
        return self

    def step(self, ids, grad):
        ts = self.ts
        B, sb, sf = self._check_onehot(ids, grad, (ts.F * ts.K, ts.K))
        if B == 0:
            return
        slot_stride = ts.K if grad.shape[1] == ts.F * ts.K and ts.F > 1 else 0
        lib = _lib.load()
        ws, need, _ = self._sort_area("SparseFtrl.step", lib.dir_sparse_adagrad_sorted_workspace_bytes, B, ts.F, ts.K)
        src = self._take_sort(ids, B, sb, sf)
        if self.packed:
            _lib.check(lib.dir_sparse_ftrl_rows_sorted_f32(_ptr(ts._ptrs), ts.F, _ptr(ids), sb, sf, _ptr(grad), grad.stride(0), slot_stride,
                                                           self.lr, self.l1, self.l2, B, _ptr(self.row_base), self.total_rows, ws, need, src,
                                                           _stream()))
        else:
            args = (_ptr(ts.ptrs), _ptr(self.acc_ptrs), _ptr(self.lin_ptrs), ts.F, ts.K, _ptr(ids), sb, sf, _ptr(grad), grad.stride(0), slot_stride,
                    self.lr, self.l1, self.l2, B, _ptr(self.row_base), self.total_rows, ws, need)
            if src is not None:
                _lib.check(lib.dir_sparse_ftrl_sorted_from_f32(*args, src, _stream()))
            else:
                _lib.check(lib.dir_sparse_ftrl_sorted_f32(*args, _stream()))
        if src is None:
            self._leave_sort(ids, B, sb, sf, ws)
        self._written()

    def step_payload(self, payload, grad, sorted_by=None):
        """Owner side of the sharded linear term's backward (shard.ShardedTables; include/dir_hip.h:
        dir_sparse_ftrl_rows_units_sorted_payload_f32): payload [n] int64 (local_row * F + slot, < 0 pruned) as received from all ranks,
        grad [n, U] fp32 in the same order, over packed rows of U = ts.units first-order terms (default 1: TableSet.ftrl_rows, grad [n]).
        sorted_by: an optimiser whose step_payload has JUST run over the same payload on this stream with the same local vocabularies
        (the SparseAdagrad of the co-located embedding rows, of any row width): its sorted (row, entry) pairs are read from its
        workspace and this call skips the key pass and the sort."""
        ts = self.ts
        U = int(getattr(ts, "units", 1))
        if not self.packed or ts.ld != 4 * U:
            raise ValueError("step_payload: packed linear training rows of 4 * units floats (TableSet.ftrl_rows)")
        n = self._check_payload(payload, grad, U, exact=False)
        if n == 0 or self.total_rows == 0:
            return
        lib = _lib.load()
        ws, need, _ = self._sort_area("SparseFtrl.step_payload", lib.dir_sparse_adagrad_sorted_workspace_bytes, n, 1, U)
        _lib.check(lib.dir_sparse_ftrl_rows_units_sorted_payload_f32(_ptr(ts._ptrs), ts.F, U, _ptr(payload), n, _ptr(grad), self.lr, self.l1,
                                                                     self.l2, _ptr(self.row_base), self.total_rows, ws, need,
                                                                     self._sorted_by("step_payload", sorted_by), _stream()))
        self._written()

    def step_bags(self, recv, P, cap_e, cap_b, grad, sorted_by=None):
        """Owner side of the first-order term's backward over sharded bags (shard.ShardedTables.lookup_bags_train(with_linear=True);
        include/dir_hip.h: dir_sparse_ftrl_rows_sorted_bags_f32): recv = the P bag slabs the forward received, grad [P*cap_b] fp32 = d lin
        of every partial-row position as received.  Entry (s, j) adds w * grad[s*cap_b + ret] to its (slot, row); every touched row takes
        one FTRL step with its summed gradient.  sorted_by: the SparseAdagrad whose step_bags has JUST run over the same slabs on this
        stream with the same local vocabularies: its sorted (row, entry) pairs are read and the key pass and the sort are skipped."""
        ts = self.ts
        if not self.packed:
            raise ValueError("step_bags: packed linear training rows (TableSet.ftrl_rows)")
        self._check_bags("step_bags", recv, P, cap_e, cap_b, grad, None)
        if self.total_rows == 0:
            return
        lib = _lib.load()
        ws, need, _ = self._sort_area("SparseFtrl.step_bags", lib.dir_sparse_adagrad_sorted_workspace_bytes, P * cap_e, 1, 1)
        _lib.check(lib.dir_sparse_ftrl_rows_sorted_bags_f32(_ptr(ts._ptrs), ts.F, _ptr(recv), P, cap_e, cap_b, _ptr(grad), self.lr, self.l1,
                                                            self.l2, _ptr(self.row_base), self.total_rows, ws, need,
                                                            self._sorted_by("step_bags", sorted_by), _stream()))
        self._written()
