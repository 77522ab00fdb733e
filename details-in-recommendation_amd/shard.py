"""shard.py -- row-sharded embedding tables with an all-to-all lookup (RCCL over xGMI on the GPU box).

Semantic precedent in the reference: min_max_variable_partitioner(max_partitions=num_ps_replicas, min_slice_size=64 << 20)
row-partitions the embedding variables and lookups resolve with partition_strategy='div'
(models/DeepFM/deepFM.py:163-167; [TF-upstream] embedding_lookup).  Here every rank of a torch.distributed group owns
contiguous 'div' row slices of the tables (by default one slice of EVERY table; `partitions=` applies the reference's
slice-count rule instead) and one lookup is, per micro-batch,

    bucket   (HIP: route every id to its owner, one fixed-capacity slab per owner -> payload slabs, inverse positions)
    exchange (all_to_all_single of the slabs, EQUAL splits: no split sizes ever reach the host)
    gather   (HIP on the owner: slab -> rows)
    exchange (all_to_all_single of the fp32 rows back, equal splits)
    finish   (HIP: the fused gather+FM kernel with "table" = the received row buffer and ids = the inverse positions:
              one pass un-permutes into [B_local, F*K] and produces the FM logit)

The batch is cut into `chunks` micro-batches on two streams, software-pipelined so that the id exchange of chunk c+1 is
issued before the row exchange of chunk c: owner gather / finish of neighbouring chunks run under the (link-bound) row
exchange.  A slab that is too small is detected on the device (overflow flag, read AFTER the whole pipeline has been
enqueued, so the stream never drains); the lookup is then repeated on the exact variable-size path (one host read of the
split sizes) and the capacity grows.  `dedup=True` sends each (slot, row) once per owner and chunk ([TF-upstream]
embedding_lookup_sparse's unique-before-gather): on skewed ids it cuts the link-bound bytes.

DeepFM's first-order weights can live on the shards too (attach_linear: slot f's weights beside slot f's embedding rows, as packed
[w | n | z | -] rows).  The linear term then rides on the same id exchange -- owner: one weight per received payload word; one float
per slab slot travels back behind the rows; requester: the sample's F weights summed in slot order -- and lookup_train(with_linear=True)
sends d logit back the same way for an owner-side FTRL step on the Adagrad step's sort of the payload.
Over multi-hot bags (lookup_bags(want_lin=True), lookup_bags_train(with_linear=True)) it rides on the bag lookup instead: the owner pools
the first-order weights of each run beside the embedding rows, one float per partial-row position travels back behind the partial rows,
and the requester applies the model's one linear_sparse_combiner.

Row groups (ShardedTables(groups=G)) store the G rows that sub-models keep for one id side by side -- the wide & deep ESMM's ctr_model and
cvr_model look up the same (slot, row) pairs (ESMM_wide_deep.py:213-217) -- so one id exchange, one owner gather and one owner-side sort
serve all of them; the finish pass de-interleaves into G outputs, the backward interleaves the G gradients again.  attach_linear([rows, U])
is the same for the first-order term: U weights behind one payload word.  ShardedESMMTrainer trains ESMM / ESMM_W_D on them (DESIGN.md
section 5.2).

DCN trains with the reference's own optimiser on the shards (enable_training_adam, ShardedDCNTrainer): TF's sparse Adam with a per-table
clip norm.  The clip norm is a property of the whole table, so the owner's step is cut in two around one all-reduce of the [F] norm shares
(an exact integer sum), and every local row moves every step, also on an owner that received nothing.  The
reference DCN's own input -- multi-hot bags with per-column combiner, weights and max_norm -- trains the same way over the bag records
the owners kept (lookup_bags_train under enable_training_adam; ShardedDCNTrainer on ragged features; section 5.3.1).

DIN's goods table lives on the shards too (ShardedDINTrainer): a sample's T history ids and its candidate are T + 1 entries of a one-slot
lookup without a finish pass, de-duplicated; the unit's kernels read the received rows through the entries' positions.  What training needs
for that is the transpose of a de-duplicated lookup -- many entry gradients summed into the one slab position they share -- as a kernel
(backend.rows_scatter_sum: lookup_train(dedup=True), lookup_rows_train / backward_rows).

xDeepFM trains on the shards as well (ShardedXDeepFMTrainer): its first-order term rides on the de-duplicated training exchange, the
gradient d lin summed per slab position by the same call and on the same sort as the row gradients (backend.rows_scatter_sum_side:
lookup_train(with_linear=True, dedup=True)).

The collectives are torch.distributed.all_to_all_single (backend "nccl" = RCCL on ROCm; "gloo" in the CPU tests).
world_size == 1 skips the collectives (unless force_collective) but still runs the three HIP steps.  The HIP steps sit
behind a small backend object so that the CPU (gloo) tests can stand the oracle in for them; the default backend is the
HIP one.
"""
import contextlib
import math
import os

import torch
import torch.distributed as dist

from . import ops

_HOST_STAGED = os.environ.get("DIR_SHARD_HOST_STAGED") == "1"
MIN_SLICE_SIZE = 64 << 20     # deepFM.py:167
MAX_GROUPS = 16               # include/dir_hip.h: dir_shard_finish_groups_f32
MAX_ROW_FLOATS = 256          # the widest row the sorted Adagrad covers (64 lanes x 16 bytes)
MAX_UNITS = 8                 # first-order terms per row (include/dir_hip.h: 1 <= units <= 8)


def refuse_shared_columns(who, columns):
    """The row shards hold one table per slot: a table that several columns share (feature_column.shared_embedding_columns) would be
    sharded as copies that train apart.  Not covered yet -- refuse by name."""
    from .feature_column import first_shared
    c = first_shared(list(columns or []))
    if c is not None:
        raise ValueError("%s: column %r shares its embedding table (collection %r) with another column; tables shared between "
                         "columns are not row-sharded yet" % (who, c.name, c.shared_embedding_collection_name))


def div_range(vocab, P, rank):
    """Rows [start, end) that `rank` owns under 'div' (first vocab % P shards hold one extra row)."""
    q, r = divmod(int(vocab), int(P))
    start = rank * (q + 1) if rank < r else r * (q + 1) + (rank - r) * q
    return start, start + (q + 1 if rank < r else q)


def partitions_for(vocab, K, max_partitions, min_slice_size=MIN_SLICE_SIZE, bytes_per_element=4):
    """[TF-upstream] partitioned_variables.min_max_variable_partitioner(max_partitions, axis=0, min_slice_size) as the reference
    calls it (models/DeepFM/deepFM.py:163-167, ESMM_wide_deep.py:213-217): a [vocab, K] variable is cut along axis 0 into
        max(1, min(vocab, max_partitions, ceil(vocab * K * bytes_per_element / min_slice_size)))
    slices (so every slice holds at least min_slice_size bytes, and num_ps_replicas = 0 leaves the variable whole).  The
    slices are the 'div' row ranges (the first vocab % n slices hold one extra row: div_range)."""
    total = int(vocab) * int(K) * int(bytes_per_element)
    return max(1, min(int(vocab), int(max_partitions), int(math.ceil(total / float(min_slice_size)))))


def place_slices(parts, P):
    """Rank of slice 0 of every table: the slices are dealt round-robin over the ranks in creation order ([TF-upstream]
    replica_device_setter's default strategy places each slice -- a variable of its own -- on the next ps task)."""
    first, nxt = [], 0
    for p in parts:
        first.append(nxt % P)
        nxt += p
    return first


def local_slice(vocab, parts, first, P, rank):
    """Rows [start, end) of a table that `rank` holds: slice j = (rank - first) mod P when j < parts, else nothing."""
    j = (rank - first) % P
    return div_range(vocab, parts, j) if j < parts else (0, 0)


def partition_layout(vocab, K, P, rank, partitions=None):
    """(parts, first, slices) of tables [vocab_f, K] over P ranks: slice count and rank of slice 0 per table, and the rows [start, end)
    of every table that `rank` holds.  partitions: None = every table cut into P slices, slice r on rank r; "reference" = the reference
    partitioner's slice-count rule (partitions_for with max_partitions = P), the slices dealt round-robin (place_slices); or an explicit
    list of slice counts, dealt the same way."""
    if partitions is None:
        parts, first = [P] * len(vocab), [0] * len(vocab)
    else:
        parts = [partitions_for(v, K, P) for v in vocab] if partitions == "reference" else [int(p) for p in partitions]
        if len(parts) != len(vocab) or any(p < 1 or p > P for p in parts):
            raise ValueError("partitions: one slice count in [1, P=%d] per table" % P)
        first = place_slices(parts, P)
    return parts, first, [local_slice(v, parts[f], first[f], P, rank) for f, v in enumerate(vocab)]


def _round_up(x, m):
    return (int(x) + m - 1) // m * m


def _lin_combiner(c):
    """The first-order term's combiner over bags: ONE name for every slot (the model's linear_sparse_combiner, deepFM.py:59)."""
    if c not in ("sum", "mean", "sqrtn"):
        raise ValueError("lin_combiner: 'sum' | 'mean' | 'sqrtn' (one for every slot), got %r" % (c,))
    return c


def _host_staged(t, group):
    """Whether a collective on `t` goes through host memory: the development transport (several ranks on ONE GPU over gloo), never on a
    multi-GPU node."""
    return _HOST_STAGED or (t.is_cuda and dist.get_backend(group) == "gloo")


def _wait(work):
    if work is not None:
        work.wait()


@contextlib.contextmanager
def _eval_mode(model):
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


class HipBackend:
    """The product path: launches of libdir_hip.so kernels."""

    def __init__(self, local_tables, vocab_dev, P, parts_dev=None, first_dev=None):
        self.ts = ops.TableSet(local_tables)
        # row policy "auto": the owner-side gather streams (non-temporal) when this rank's shards exceed the
        # Infinity Cache, like the single-GPU gather
        self.vocab_dev = vocab_dev
        self.P = P
        self.parts_dev, self.first_dev = parts_dev, first_dev
        self._back = None
        self._back_key = None         # rows_as_tables' key of the exact path's last row buffer
        self.lin_ts, self._ftrl, self.U = None, None, 1      # attach_linear

    # ---- variable-size (exact) path -----------------------------------------------------------------------
    def bucket(self, flat_ids):
        return ops.shard_bucket(flat_ids, self.vocab_dev, self.P, parts=self.parts_dev, first=self.first_dev)

    def gather_packed(self, payload):
        return ops.gather_packed(self.ts, payload)

    def make_optimizer(self, lr, initial_accumulator_value):
        return ops.SparseAdagrad(self.ts, lr, initial_accumulator_value)

    def apply_adagrad(self, opt, payload, grad_rows):
        opt.step_payload(payload, grad_rows)                     # HIP: sorted (row, entry) pairs, per-tile segmented reduce

    # ---- owner-side sparse Adam (ShardedTables.enable_training_adam): the step in two halves around the ranks' norm exchange ----
    def make_adam(self, beta1, beta2, eps, clip_norm):
        return ops.SparseAdam(self.ts, beta1, beta2, eps, clip_norm)

    def adam_norm(self, opt, payload, grad_rows):
        """-> [F] int64: this owner's share of every table's ||g||^2, 2^-32 fixed point (HIP: the payload's sort + the norm pass)."""
        return opt.norm_payload(payload, grad_rows)

    def adam_apply(self, opt, payload, grad_rows, norm2_global):
        """The touched rows on the norm pass's sort, clipped with the GLOBAL norms ([F] float64, None without a clip), then the decay
        pass over every other local row."""
        opt.step_payload(payload, grad_rows, norm2_global)

    def back_buffer(self, n, K, device):
        if self._back is None or self._back.shape[0] != n:
            self._back = torch.empty((n, K), dtype=torch.float32, device=device)
        return self._back

    def finish(self, back, inv, B, F, want_fm, out=None, fm=None):
        key = _rows_key(back, F)
        if key != self._back_key:     # the exact path's buffer moved (training: a fresh one per lookup): the view of the last one goes
            _ROWS_TS.pop(self._back_key, None)     # with it, or the cache would pin every buffer it has ever seen
            self._back_key = key
        return self.finish_chunk(back, inv.view(B, F), want_fm, out, fm)

    # ---- fixed-capacity path ------------------------------------------------------------------------------
    def new_workspace(self, device):
        return torch.zeros(128, dtype=torch.int32, device=device)      # dir_shard_bucket_cap_workspace_bytes: slab counters + arrival counter

    def bucket_cap(self, ids2d, cap, payload, inv, counts, overflow, workspace, stat=None, dedup=False):
        """ids2d [Bc, F] -> slabs (packed headers) + inv; dedup: inv comes back field-major (inv2d() gives the [Bc, F] view)."""
        if dedup:
            ops.shard_bucket_cap_dedup(ids2d, self.vocab_dev, self.P, cap, payload, inv, counts, overflow, workspace,
                                       parts=self.parts_dev, first=self.first_dev, stat=stat)
        else:
            ids2d = ids2d if ids2d.is_contiguous() else ids2d.contiguous()
            ops.shard_bucket_cap(ids2d.reshape(-1), self.vocab_dev, self.P, cap, payload, inv, counts, overflow, workspace,
                                 parts=self.parts_dev, first=self.first_dev, stat=stat)

    @staticmethod
    def inv2d(inv, Bc, F, dedup):
        return inv.view(F, Bc).t() if dedup else inv.view(Bc, F)

    def slab_stat(self, recv_all, n_slabs, cap, stat):
        ops.shard_slab_stat(recv_all, n_slabs, cap, stat)

    def gather_slabs(self, recv, cap, out):
        ops.gather_slabs(self.ts, recv, self.P, cap, out)

    def finish_chunk(self, back, inv2d, want_fm, out=None, fm=None):
        ts = rows_as_tables(back, inv2d.shape[1])
        if want_fm:
            return ops.gather_fm(ts, inv2d, out=out, fm=fm)
        return ops.embedding_bag(ts, inv2d, out=out), None

    def rows_scatter_sum(self, idx, vals, R, out):
        """Requester, backward: out [R, K] = the rows of vals [n, K] summed per position idx [n] (< 0: dropped), zeros where nobody
        points -- the transpose of reading `out` through idx, also when many entries share a position (a de-duplicated lookup).
        HIP: sorted, compensated run sums, no float atomics; a position named once gets its entry's row bit for bit."""
        ops.rows_scatter_sum(idx, vals, R, out=out)

    def rows_scatter_sum_side(self, idx, vals, side, side_div, R, out, out_side):
        """rows_scatter_sum plus, on the same sort, out_side [R, U] = side [.., U] row i // side_div summed per position idx[i]: the
        first-order term's gradient of a de-duplicated lookup (side = d lin [Bc, U], side_div = F), read in place."""
        ops.rows_scatter_sum_side(idx, vals, side, side_div, R, out=out, out_side=out_side)

    # ---- row groups (ShardedTables(groups=G), G > 1): the finish pass that de-interleaves, and its transpose --------
    def finish_groups(self, back, inv2d, K, outs):
        """Requester: back [n, G*K], inv2d [Bc, F] -> outs[g][b, f*K:(f+1)*K] = group g's piece of row inv2d[b, f] (zeros where < 0);
        every received row is read once."""
        ops.shard_finish_groups(back, inv2d, K, outs)

    def grad_groups(self, grads, inv2d, K, send):
        """Requester, backward: send [n, G*K] zero-filled, then row inv2d[b, f] = the entry's G gradient pieces side by side."""
        ops.shard_grad_groups(grads, inv2d, K, send)

    # ---- multi-hot bags, pooled on the owner (lookup_bags) ------------------------------------------------
    def new_bags_workspace(self, device):
        return torch.zeros(256, dtype=torch.int32, device=device)      # dir_shard_bags_workspace_bytes: 1024 bytes

    def bags_bucket(self, values, offsets, weights, B, sb, sf, combiner, flags, cap_e, cap_b, slabs, pos, mask, denom, workspace):
        slot_comb, comb = ops.slot_combiners(self.ts, combiner)
        ops.shard_bags_bucket(values, offsets, weights, B, sb, sf, self.vocab_dev, self.P, slot_comb, comb, flags, cap_e, cap_b, slabs, pos,
                              mask, denom, workspace, parts=self.parts_dev, first=self.first_dev)

    def bags_pool(self, recv, cap_e, cap_b, max_norm, rows, stat=None):
        slot_mn, mn = ops.slot_max_norms(self.ts, max_norm)
        ops.shard_bags_pool(self.ts, recv, self.P, cap_e, cap_b, slot_mn, mn, rows, stat=stat)

    def bags_combine(self, back, cap_b, pos, mask, denom, B, combiner, out, fm=None):
        slot_comb, comb = ops.slot_combiners(self.ts, combiner)
        ops.shard_bags_combine(back, self.P, pos, mask, denom, B, self.ts.F, slot_comb, comb, out, fm=fm)

    # ---- their backward (lookup_bags_train) ----
    def bags_grad(self, g, cap_b, pos, mask, denom, B, combiner, send):
        """Requester: g [B, F*K] -> c_bag * g[b, f] at every partial row the forward received (send [P*cap_b, K])."""
        slot_comb, comb = ops.slot_combiners(self.ts, combiner)
        ops.shard_bags_grad(g, self.P, pos, mask, denom, B, self.ts.F, slot_comb, comb, cap_b, send)

    def bags_adagrad(self, opt, recv, cap_e, cap_b, grad_rows, max_norm):
        """Owner: the sorted Adagrad over the received bag records, entry gradient w * grad_rows[src*cap_b + ret]."""
        slot_mn, mn = ops.slot_max_norms(self.ts, max_norm)
        opt.step_bags(recv, self.P, cap_e, cap_b, grad_rows, slot_mn, mn)

    # ... under enable_training_adam: the two halves of the owner's Adam step over the same records
    def bags_adam_norm(self, opt, recv, cap_e, cap_b, grad_rows, max_norm):
        """-> [2, F] int64: this owner's share of every table's ||g||^2 (the norm words, as adam_norm), g = the rows' summed record
        gradients through the max_norm clip derivative (HIP: the records' sort + the norm pass)."""
        slot_mn, mn = ops.slot_max_norms(self.ts, max_norm)
        return opt.norm_bags(recv, self.P, cap_e, cap_b, grad_rows, slot_mn, mn)

    def bags_adam_apply(self, opt, recv, cap_e, cap_b, grad_rows, max_norm, norm2_global):
        """The touched rows on the norm pass's sort, clipped with the GLOBAL norms ([F] float64, None without a clip), then the decay
        pass over every other local row."""
        slot_mn, mn = ops.slot_max_norms(self.ts, max_norm)
        opt.step_bags(recv, self.P, cap_e, cap_b, grad_rows, norm2_global, slot_mn, mn)

    # ---- the first-order (linear) term, co-located with the embedding rows (ShardedTables.attach_linear) -------------
    def attach_linear(self, rows, arena):
        """rows[f]: this rank's packed [local rows, 4 U] rows of one arena: U blocks [w | n | z | -], one per first-order term (unit) of
        the row (U = 1: TableSet.ftrl_rows' layout).  The four steps below carry U floats per entry; the views here are unit 0's."""
        U = self.U = rows[0].shape[1] // 4
        ts = ops.TableSet([r[:, 0:1] for r in rows], ld=4 * U)
        ts.accums = [r[:, 1:2] for r in rows]
        ts.linears = [r[:, 2:3] for r in rows]
        ts.arena, ts.rows, ts.units = arena, rows, U
        self.lin_ts, self._ftrl = ts, None

    def linear_gather(self, recv, cap, out):
        """Owner: out[i*U + u] = unit u's weight of received payload word i (cap: the slab capacity, None: recv is a flat payload); every
        word of out is written."""
        ops.shard_linear_gather(self.lin_ts, recv, self.P, cap, out)

    def linear_finish(self, wback, inv2d, bias, out):
        """Requester: out [Bc, U], column u = sum_f wback[inv2d[b, f]*U + u] + bias[u], ops.linear_logit's sum bit for bit."""
        ops.shard_linear_finish(wback, inv2d, bias, out, units=self.U)

    def linear_grad(self, g, inv2d, send):
        """Requester, backward: send zero-filled, then send[inv2d[b, f]*U + u] = g[b, u]."""
        ops.shard_linear_grad(g, inv2d, send, units=self.U)

    def apply_ftrl(self, payload, grad, lr, l1, l2, sorted_by=None):
        """Owner, backward: the sorted FTRL over the payload it kept, grad [n, U] in payload order; sorted_by = the Adagrad optimiser that
        has just sorted the same payload (apply_adagrad): its sorted pairs are reused and the second key pass and sort are skipped."""
        self._ftrl_opt(lr, l1, l2).step_payload(payload, grad, sorted_by=sorted_by)

    def _ftrl_opt(self, lr, l1, l2):
        o = self._ftrl
        if o is None or (o.lr, o.l1, o.l2) != (float(lr), float(l1), float(l2)):
            o = self._ftrl = ops.SparseFtrl(self.lin_ts, lr, l1=l1, l2=l2)
        return o

    def ftrl_dense(self, w, accum, linear, grad, lr, l1, l2):
        """FTRL step of a replicated dense variable (the linear bias) with its summed gradient."""
        ops.ftrl_dense_(w, accum, linear, grad, lr, l1, l2)

    # ---- ... over multi-hot bags: it rides on the bag lookup (lookup_bags(want_lin=True), lookup_bags_train(with_linear=True)) ------
    def bags_linear_pool(self, recv, cap_e, cap_b, out):
        """Owner: out [P*cap_b] = the first-order weights of every run pooled as sum w_e * weight, in entry order; every word is written."""
        ops.shard_bags_linear_pool(self.lin_ts, recv, self.P, cap_e, cap_b, out)

    def bags_linear_combine(self, lback, cap_b, pos, mask, values, offsets, weights, B, sb, sf, flags, combiner, lden, bias, out):
        """Requester: out [B, 1] = sum_f combiner(bag (b, f)'s partials in ascending owner order) + bias; mean / sqrtn write lden [B*F]
        (the linear combiner's denominators, from the CSR entries with the lookup's liveness rule) on the way."""
        ops.shard_bags_linear_combine(lback, self.P, cap_b, pos, mask, values, offsets, weights, sb, sf, self.vocab_dev, flags, B, self.ts.F,
                                      combiner, lden, bias, out)

    def bags_linear_grad(self, g, cap_b, pos, mask, lden, B, combiner, send):
        """Requester, backward: send[pos of every partial the forward received] = g[b] (/ lden for mean and sqrtn)."""
        ops.shard_bags_linear_grad(g, self.P, cap_b, pos, mask, lden, B, self.ts.F, combiner, send)

    def bags_ftrl(self, recv, cap_e, cap_b, grad, lr, l1, l2, sorted_by=None):
        """Owner, backward: the sorted FTRL over the bag records it kept, entry gradient w * grad[src*cap_b + ret]; sorted_by = the Adagrad
        optimiser that has just sorted the same slabs (bags_adagrad): its sorted pairs are reused."""
        self._ftrl_opt(lr, l1, l2).step_bags(recv, self.P, cap_e, cap_b, grad, sorted_by=sorted_by)


_ROWS_TS = {}


def _rows_key(rows, F):
    return rows.data_ptr(), rows.shape[0], rows.shape[1], F


def rows_as_tables(rows, F, absmax=None):
    """A received row buffer -- of a lookup_consume() micro-batch, or of the lookup's own finish pass (HipBackend.finish / finish_chunk) --
    as a TableSet of F identical "tables" (one per slot), cached by address: what ops.gather_fm / ops.embedding_bag /
    ops.tower(gather=...) take as their tables, with the inverse positions as ids.  (The gathers never read TableSet.absmax -- only
    TableSet.range_ok and ops.tower do -- so an absmax= left on an entry by one caller changes nothing a finish pass computes.)
    absmax: the largest |value| of the SHARDED tables (ShardedTables.absmax()): the magnitude bound a kernel that picks its split
    arithmetic by the tables' range (ops.tower(split=None)) must see -- the buffer's own contents change with every lookup, behind the
    back of TableSet.absmax()'s version-keyed cache."""
    key = _rows_key(rows, F)
    ts = _ROWS_TS.get(key)
    if ts is None:
        if len(_ROWS_TS) > 192:      # (room for the views of every live plan's buffers, the finish passes' and the consumers' alike)
            _ROWS_TS.clear()
        ts = _ROWS_TS[key] = ops.TableSet([rows] * F)
        ts.row_policy = "reuse"      # just received: largely cache-resident
    if absmax is not None:
        ts.absmax = lambda every=1, _v=float(absmax): _v
    return ops.held(ts)              # a graph captured now reads its pointer array: the capture's hold keeps it past the clear() above


class _Plan:
    """Persistent buffers of the fixed-capacity pipeline for one (local batch size, buffer slot, slab capacity): stable addresses,
    so nothing is allocated per lookup and a lookup can be captured in a HIP graph.  Only the slab capacity has to agree across
    the ranks (equal-split exchanges); everything sized by the batch is local."""

    def __init__(self, st, B, cap, train=False):
        dev, P, F, K = st.device, st.P, st.F, st.KW     # (KW: the stored row, G * K floats with row groups)
        self.B, self.cap = B, cap
        self.train = train            # the training pipeline's plan: its verdicts move _cap_train, not _cap (_learn)
        self.slot = None              # which capacity the plan's slabs follow (_plan)
        self.dedup = False            # a de-duplicated training plan: positions shared by many entries (the backward sums into them)
        self.P, self.device, self.lrows = P, dev, None
        C = self.C = st._C()
        per = -(-B // C) if B else 0
        self.bounds = [(min(B, c * per), min(B, (c + 1) * per)) for c in range(C)]       # a chunk may be empty (B < C)
        i64 = dict(dtype=torch.int64, device=dev)
        alias = not st._collective()                     # one rank, no collectives: receive buffers ARE the send buffers
        slab = P * (cap + 1)
        self.send_all = torch.empty(C * slab, **i64)
        self.recv_all = self.send_all if alias else torch.empty(C * slab, **i64)
        self.send = [self.send_all[c * slab:(c + 1) * slab] for c in range(C)]
        self.recv = [self.recv_all[c * slab:(c + 1) * slab] for c in range(C)]
        self.inv = [torch.empty(max(1, (e - s) * F), **i64)[:(e - s) * F] for s, e in self.bounds]
        self.counts = torch.zeros((C, P), **i64)
        self.flags = torch.zeros((C, 1), dtype=torch.int32, device=dev)
        self.ws = [st.backend.new_workspace(dev) for _ in range(C)]
        # one matrix for all micro-batches (chunk c's positions start at c * P * cap): lookup_rows_train hands it out whole, and a consumer
        # that needs the whole local batch in ONE kernel call (ShardedDINTrainer.predict) reads it through offset positions
        # (zeros once, here: a consumer that reads position 0 for a pruned id and multiplies by 0 -- the DIN unit's candidate row -- must
        # never meet the NaNs of uninitialised memory behind a slab's valid rows)
        self.rows_all = torch.zeros((C * P * cap, K), dtype=torch.float32, device=dev)
        self.back_all = self.rows_all if alias else torch.zeros_like(self.rows_all)
        self.rows = [self.rows_all[c * P * cap:(c + 1) * P * cap] for c in range(C)]
        self.back = [self.back_all[c * P * cap:(c + 1) * P * cap] for c in range(C)]
        self.cstat = torch.zeros((C, 2), **i64)           # per chunk [overflow, max demand] of THIS rank (diagnostic)
        self.stat = torch.zeros(2, **i64)                 # ... over all chunks and ranks, read off the received slab headers
        self.host = torch.empty(2, dtype=torch.int64, pin_memory=dev.type == "cuda")
        self.fin = None                                   # events behind the last enqueued lookup's final kernels (one per side stream)

    def lin_buffers(self, U=1):
        """The linear term's buffers, made at the first lookup that wants it: U floats (units) per slab slot and micro-batch, sent (lrows)
        and received (lback); [C, P*cap*U] each, so that the backward hands all micro-batches to the owner's update as one array in payload order."""
        if self.lrows is None or self.lrows_all.shape[1] != self.P * self.cap * U:
            n = self.P * self.cap * U
            self.lrows_all = torch.zeros((self.C, n), dtype=torch.float32, device=self.device)
            self.lback_all = self.lrows_all if self.recv_all is self.send_all else torch.zeros_like(self.lrows_all)
            self.lrows = [self.lrows_all[c] for c in range(self.C)]
            self.lback = [self.lback_all[c] for c in range(self.C)]
        return self.lrows, self.lback


class _BagPlan:
    """Persistent buffers of lookup_bags for one (local batch size, entry capacity, pair capacity): stable addresses, so that a lookup can
    be captured in a HIP graph after one eager call.  Only the two capacities have to agree across the ranks.
    train: a plan of lookup_bags_train -- `busy` from a forward to its backward, and pinned host words of its own for the verdict."""

    def __init__(self, st, B, cap_e, cap_b, train=False):
        dev, P, F, K = st.device, st.P, st.F, st.K
        self.cap_e, self.cap_b = cap_e, cap_b
        self.busy = False
        self.host = torch.empty(3, dtype=torch.int64, pin_memory=True) if train and dev.type == "cuda" else None
        i64 = dict(dtype=torch.int64, device=dev)
        alias = not st._collective()                     # one rank, no collectives: receive buffers ARE the send buffers
        self.send = torch.empty(P * (cap_e + 1) * 2, **i64)         # P slabs of (cap_e + 1) 16-byte records
        self.recv = self.send if alias else torch.empty_like(self.send)
        nb = B * F
        self.pos = torch.empty(max(1, nb * P), dtype=torch.int32, device=dev)
        self.mask = torch.empty(max(1, nb), **i64)
        self.denom = torch.empty(max(1, nb), dtype=torch.float32, device=dev)
        self.rows = torch.empty((P * cap_b, K), dtype=torch.float32, device=dev)
        self.back = self.rows if alias else torch.empty_like(self.rows)
        self.ws = st.backend.new_bags_workspace(dev)
        self.stat = torch.zeros(3, **i64)                 # [overflow, largest entry demand, largest pair demand], off the received headers
        self.P, self.nb, self.device, self.lrows = P, nb, dev, None

    def lin_buffers(self):
        """The first-order term's buffers, made at the first lookup that wants it: one float per partial-row position, sent (lrows) and
        received (lback; the same at world 1), and the linear combiner's denominator per bag (lden: written by mean / sqrtn forwards, read
        by their backward).  -> (lrows, lback, lden)"""
        if self.lrows is None:
            self.lrows = torch.zeros(self.P * self.cap_b, dtype=torch.float32, device=self.device)
            self.lback = self.lrows if self.recv is self.send else torch.zeros_like(self.lrows)
            self.lden = torch.ones(max(1, self.nb), dtype=torch.float32, device=self.device)
        return self.lrows, self.lback, self.lden


class _Lookup:
    """A lookup whose pipeline has been enqueued (on the side streams on a GPU).  result() makes the caller's stream wait for it,
    applies the overflow policy and returns emb (or (emb, fm)).  Issue the NEXT lookup before calling result() -- or before the
    compute that consumes this one -- and the exchange runs under that compute."""

    def __init__(self, st, plan, ids, want_fm, out, fm, done, consumer=None, lin=None):
        """plan None: the lookup ran on the exact path, on the caller's stream -- out / fm / lin are complete, nothing is left to check."""
        self.st, self.plan, self.ids, self.want_fm, self.out, self.fm, self.done = st, plan, ids, want_fm, out, fm, done
        self.consumer = consumer
        self.lin = lin                # None, or (lin [B, 1], bias | None): the first-order term rides along (want_lin)
        self.fin = plan.fin if plan is not None else None      # this lookup's completion events on the side streams
        self.joined = plan is None
        self.checked = plan is None or done is False

    def join(self):
        """The caller's stream waits for THIS lookup's last kernels (events recorded when it was enqueued), not for whatever else has
        been queued on the side streams since: a later lookup keeps running under the compute that follows."""
        if not self.joined:
            self.joined = True
            if self.fin:
                cur = torch.cuda.current_stream(self.st.device)
                for e in self.fin:
                    cur.wait_event(e)

    def result(self):
        st = self.st
        self.join()
        if not self.checked and st.check == "eager":
            self.checked = True
            over, demand = st._read_flags(self.plan, self.done)
            st._learn(self.plan, over, demand)
            if over:                                          # rare: repeat on the exact path (results overwrite out / fm in stream order)
                st.stats["fallbacks"] += 1
                st._lookup_exact(self.ids, self.want_fm, out=self.out, fm=self.fm, consumer=self.consumer, lin=self.lin)
        res = (self.out,) + ((self.fm,) if self.want_fm else ()) + ((self.lin[0],) if self.lin is not None else ())
        return res if len(res) > 1 else self.out              # emb | (emb, fm) | (emb, lin) | (emb, fm, lin); emb = None under a consumer


class _RowsLookup:
    """Handle of ShardedTables.lookup_rows_async."""

    def __init__(self, lk, chunks):
        self.lk, self.chunks = lk, chunks

    def result(self):
        self.lk.result()
        self.lin = self.lk.lin[0] if self.lk.lin is not None else None        # the first-order term [B, 1] (want_lin), after any repair
        return list(self.chunks)


class _RowsTrainLookup:
    """Handle of ShardedTables.lookup_rows_train: .rows [R, K] (the received rows of all micro-batches, one matrix), .inv [B, F] int64 (every
    entry's position in .rows, < 0: pruned) and backward_rows, which runs exactly once."""

    def __init__(self, st, saved, rows, inv):
        self.st, self.saved, self.rows, self.inv = st, saved, rows, inv

    def backward_rows(self, idx, grad_rows):
        """idx [m] int64: positions in .rows (< 0: dropped; any order, any number of entries per position); grad_rows [m, K]: d loss / d
        .rows[idx[i]] of entry i.  The entries of a position are summed in entry order (backend.rows_scatter_sum), the slabs travel the
        forward's row exchange backwards and every owner takes its optimiser step (Adagrad, or Adam with its norm exchange): one
        synchronous step over the global batch.  Every rank must call it (SPMD), exactly once per lookup."""
        if self.saved is None:
            raise RuntimeError("backward_rows: this lookup's backward has run already")
        st, saved = self.st, self.saved
        self.saved = None
        K = st.K
        if grad_rows.dim() != 2 or grad_rows.shape[1] != K or idx.dim() != 1 or idx.shape[0] != grad_rows.shape[0]:
            raise ValueError("backward_rows: idx [m] and grad_rows [m, K=%d]" % K)
        st._refuse_adam_capture(grad_rows)
        R = int(self.rows.shape[0])
        slabs = torch.empty((R, K), dtype=torch.float32, device=self.rows.device)
        if grad_rows.shape[0] and grad_rows.stride(1) != 1:
            grad_rows = grad_rows.contiguous()
        st.backend.rows_scatter_sum(idx.contiguous(), grad_rows, R, slabs)
        st._backward_apply(saved, None, slabs=slabs)


class ShardedTables:
    """This rank's row slices of F tables [vocab_f, K].

    partitions: None = every table cut into P slices, slice r on rank r (the north star's row sharding); "reference" = the
      reference partitioner's slice-count rule (partitions_for with max_partitions = P) with the slices dealt round-robin; or an
      explicit list of slice counts.  local_tables[f] holds local_slice(...) rows of table f (possibly zero rows).
    chunks: micro-batches per lookup when there is an exchange to hide (pipelined on two streams; every collective costs
      host time, so 2 by default; without collectives -- one rank -- a lookup is ONE chunk on the caller's stream);
    slack: slab capacity = ceil(slack * n / P) entries per owner and chunk (None: n / P + 8 sigma of the binomial count + 64:
      ~3 % padding at 16 384 x 26 ids over 8 ranks);  max_batch: the largest local batch any rank will look up (sizes the slabs;
      default: the first lookup's batch, MAX over the ranks);
    mode: "auto" (fixed capacity, exact fallback on overflow; switches to "exact" when the owners' demand is so uneven that
      padding would cost more than the host read), "fixed", "exact";
    check: "eager" (result() reads the overflow verdict: no wait when the next lookup was issued first; an overflow is repaired on
      the exact path), "lazy" (a lookup's verdict is read right after the NEXT lookup has been enqueued; an overflow raises),
      "never" (graph capture; call check_overflow() yourself);
    dedup: send each (slot, row) once per owner, chunk and 2048/4096-sample tile (csrc/ids.hip: bucket_cap_dedup_k);
    side_cus: confine the lookup's side streams to that many compute units each (for lookups prefetched under MFMA-bound compute).
    groups: G rows of K floats stored side by side for every (slot, local row) -- local_tables[f] is [local rows, G*K], the wide & deep
      ESMM's [ctr row | cvr row] (from_full_groups).  One id exchange and one owner gather serve every group;
      lookup / lookup_async / lookup_train return a TUPLE of G tensors [B_local, F*K] where they return one tensor at G = 1.  One-hot
      lookups only: want_fm, lookup_consume, lookup_rows and the bag forms raise NotImplementedError.  K % 4 == 0, G <= 16, G*K <= 256.

    Ranks may look up DIFFERENT local batch sizes (an uneven last batch): the only quantity the equal-split exchanges need to agree
    on is the slab capacity, which is agreed once (first lookup: one host MAX) and afterwards changes only on statistics every rank
    reads identically off the slab headers.  Every rank must call lookup the same number of times (SPMD)."""

    def __init__(self, local_tables, vocab, group=None, backend=None, force_collective=False, partitions=None, chunks=2,
                 slack=None, mode="auto", check="eager", dedup=False, max_batch=None, side_cus=None, groups=1):
        self.group = group
        self.force_collective = force_collective  # issue the all_to_all calls even when world_size == 1
        self.P = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.vocab = [int(v) for v in vocab]
        self.F = len(self.vocab)
        self.local_tables = list(local_tables)
        self.G = int(groups)
        self.KW = int(self.local_tables[0].shape[1])     # floats of a stored row: G * K
        if self.G < 1 or self.KW % self.G:
            raise ValueError("groups=%d: the tables' rows of %d floats must hold `groups` rows of one width" % (self.G, self.KW))
        self.K = self.KW // self.G
        if self.G > 1:
            if self.K % 4:
                raise ValueError("groups=%d: K=%d must be a multiple of 4 (the grouped finish pass moves 16-byte pieces)" % (self.G, self.K))
            if self.G > MAX_GROUPS or self.KW > MAX_ROW_FLOATS:
                raise ValueError("groups=%d x K=%d: at most %d groups and rows of %d floats (what the owner gather and the sorted Adagrad "
                                 "cover)" % (self.G, self.K, MAX_GROUPS, MAX_ROW_FLOATS))
        self.U = 1                    # attach_linear: first-order terms (units) per row
        P = self.P
        self.parts, self.first, self.slices = partition_layout(self.vocab, self.K, P, self.rank, partitions)   # slices: this rank's [start, end)
        for f, (t, (s, e)) in enumerate(zip(self.local_tables, self.slices)):
            if t.shape[0] != e - s:
                raise ValueError("table %d: rank %d must hold rows [%d,%d) (%d rows), got %d" % (f, self.rank, s, e, e - s, t.shape[0]))
        self.device = self.local_tables[0].device
        self.vocab_dev = torch.tensor(self.vocab, dtype=torch.int64, device=self.device)
        custom = partitions is not None
        self.parts_dev = torch.tensor(self.parts, dtype=torch.int32, device=self.device) if custom else None
        self.first_dev = torch.tensor(self.first, dtype=torch.int32, device=self.device) if custom else None
        self.backend = backend or HipBackend(self.local_tables, self.vocab_dev, P, self.parts_dev, self.first_dev)
        if mode not in ("auto", "fixed", "exact") or check not in ("eager", "lazy", "never"):
            raise ValueError("mode: auto | fixed | exact; check: eager | lazy | never")
        self.chunks, self.slack, self.mode, self.check, self.dedup = max(1, int(chunks)), slack, mode, check, bool(dedup)
        self.max_batch = max_batch
        self.side_cus = side_cus      # None: ordinary side streams; n: the lookup's two side streams are confined to n CUs each
        self._plans = {}
        self._cap = None              # the agreed slab capacity (collective mode); _cap0: its first value (the no-skew demand)
        self._cap_train = None        # the training pipeline's own capacity (never shrunk by de-duplicated inference verdicts)
        self._cap_train_dedup = None  # ... and the de-duplicated training pipeline's (shrinks to what de-duplication leaves of a micro-batch)
        self._cap0 = None
        self._share0 = None           # an owner's share of a micro-batch without skew (_agree_cap)
        self._use_exact = mode == "exact"
        self._unchecked = []          # lookups whose overflow verdict has not been read yet (check = lazy / never)
        self._slot = 0
        self._inflight = {}
        self._streams = None          # the two side streams of the pipeline and the verdict's stream (_ensure_streams)
        self._chk_stream = None
        self.optimizer = None         # enable_training: the owner-side sparse Adagrad; enable_training_adam: the owner-side sparse Adam
        self._adam = False
        self.stats = {"lookups": 0, "fallbacks": 0, "cap": None}
        self._updates = 0             # owner-side optimiser steps applied so far (the same on every rank: absmax()'s collective decision)
        self._absmax_all = None
        self._bag_cap = None          # lookup_bags: the agreed (entry, partial-row) slab capacities -- separate from the one-hot ones
        self._bag_plans = {}
        self._bag_unchecked = []      # lookup_bags verdicts not read yet (check = lazy / never): (event | None, host words)
        self._bag_hosts, self._bag_host_i = None, 0
        self._bag_train_plans = {}    # lookup_bags_train's own plans: an inference lookup_bags between a forward and its backward never
                                      # touches the slabs, pos, mask and denom that backward reads
        self.lin_rows = None          # attach_linear: this rank's packed first-order rows [local rows, 4] = [w | n | z | -], one per slot
        self._lin_arena = None        # ... and the one allocation they are blocks of
        self._lin_hp = None           # enable_linear_training: (lr, l1, l2) of the owner-side FTRL

    @classmethod
    def from_full(cls, full_tables, group=None, **kw):
        """Slice replicated full tables down to this rank's shard (tests / small cases)."""
        P = dist.get_world_size(group) if dist.is_initialized() else 1
        rank = dist.get_rank(group) if dist.is_initialized() else 0
        vocab = [t.shape[0] for t in full_tables]
        _, _, slices = partition_layout(vocab, full_tables[0].shape[1], P, rank, kw.get("partitions"))
        return cls([t[s:e].contiguous() for t, (s, e) in zip(full_tables, slices)], vocab, group=group, **kw)

    @classmethod
    def from_full_groups(cls, full_tables_per_group, group=None, **kw):
        """from_full for row groups: full_tables_per_group[g][f] is group g's replicated table [vocab_f, K] (for ESMM: [ctr_model's tables,
        cvr_model's]); this rank's slices of the G tables of a slot are stored side by side, [local rows, G*K]."""
        per = [list(t) for t in full_tables_per_group]
        G, t0 = len(per), per[0]
        for g, tg in enumerate(per):
            if len(tg) != len(t0) or any(a.shape != b.shape for a, b in zip(tg, t0)):
                raise ValueError("from_full_groups: group %d's tables must have group 0's shapes" % g)
        P = dist.get_world_size(group) if dist.is_initialized() else 1
        rank = dist.get_rank(group) if dist.is_initialized() else 0
        vocab = [t.shape[0] for t in t0]
        _, _, slices = partition_layout(vocab, t0[0].shape[1], P, rank, kw.get("partitions"))
        local = [torch.cat([tg[f][s:e] for tg in per], dim=1).contiguous() for f, (s, e) in enumerate(slices)]
        return cls(local, vocab, group=group, groups=G, **kw)

    def group_tables(self, g):
        """Group g's rows of this rank's shard: one [local rows, K] strided VIEW of local_tables[f] per slot."""
        if not 0 <= g < self.G:
            raise ValueError("group %d of %d" % (g, self.G))
        return [t[:, g * self.K:(g + 1) * self.K] for t in self.local_tables]

    def group_accums(self, g):
        """Group g's Adagrad accumulators (enable_training first): [local rows, K] views, like group_tables."""
        if self.optimizer is None or self._adam:
            raise RuntimeError("call enable_training(lr) first")
        if not 0 <= g < self.G:
            raise ValueError("group %d of %d" % (g, self.G))
        accs = self.optimizer.accums if hasattr(self.optimizer, "accums") else self.backend.accums(self.optimizer)
        return [a[:, g * self.K:(g + 1) * self.K] for a in accs]

    def _no_groups(self, what):
        if self.G > 1:
            raise NotImplementedError("%s is not available on grouped tables (groups=%d): row groups cover the one-hot lookup, lookup_async and "
                                      "lookup_train only" % (what, self.G))

    # ---- the first-order (linear) term: slot f's weights live beside slot f's embedding rows ---------------------------
    def attach_linear(self, local_weights, initial_accumulator_value=0.1):
        """Give the shards DeepFM's first-order weights (the reference creates them under the same partitioner as the embedding tables:
        deepFM.py:206-209 beside :163-175).  local_weights[f]: this rank's slice of slot f's weights -- the rows local_slice(...) gives, i.e.
        as many as local_tables[f] has; shape [rows] or [rows, 1].  They are stored as packed 16-byte training rows [w | n | z | -]
        (TableSet.ftrl_rows' layout; n = initial_accumulator_value, z = 0), co-located with the embedding rows: the linear term then
        rides on the embedding lookup's id exchange (lookup(want_lin=True), lookup_train(with_linear=True))."""
        local_weights = list(local_weights)
        if len(local_weights) != self.F:
            raise ValueError("attach_linear: one weight vector per table (F=%d), got %d" % (self.F, len(local_weights)))
        n_rows = [int(t.shape[0]) for t in self.local_tables]
        U = int(local_weights[0].shape[1]) if local_weights[0].dim() == 2 else 1
        if not 1 <= U <= MAX_UNITS:
            raise ValueError("attach_linear: units = %d (1 <= units <= %d)" % (U, MAX_UNITS))
        for f, w in enumerate(local_weights):
            if w.numel() != n_rows[f] * U or w.dim() > 2 or (w.dim() == 2 and w.shape[1] != U):
                raise ValueError("attach_linear: slot %d: rank %d holds %d rows, got weights of shape %s (units = %d)"
                                 % (f, self.rank, n_rows[f], tuple(w.shape), U))
        # units = U: U blocks [w | n | z | -] per row, side by side (16 U bytes; U = 1: TableSet.ftrl_rows' layout)
        arena = torch.zeros(sum(n_rows) * 4 * U + 4, dtype=torch.float32, device=self.device)
        off = (-(arena.data_ptr() // 4)) % 4               # rows 16-byte aligned
        rows = []
        for w, v in zip(local_weights, n_rows):
            blk = arena[off:off + v * 4 * U].view(v, 4 * U)
            blk[:, 0::4] = w.detach().reshape(v, U).to(device=self.device, dtype=torch.float32)
            blk[:, 1::4] = float(initial_accumulator_value)
            rows.append(blk)
            off += v * 4 * U
        self.lin_rows, self._lin_arena, self.U = rows, arena, U
        attach = getattr(self.backend, "attach_linear", None)
        if attach is not None:
            attach(rows, arena)
        return self

    def attach_linear_from_full(self, full_weights, initial_accumulator_value=0.1):
        """attach_linear from replicated full weights ([vocab_f], [vocab_f, 1] or, units = U, [vocab_f, U]), sliced as from_full slices
        the tables."""
        return self.attach_linear([(w if w.dim() == 2 and w.shape[1] > 1 else w.reshape(-1))[s:e] for w, (s, e) in zip(full_weights, self.slices)],
                                  initial_accumulator_value)

    def _need_linear(self, what):
        if self.lin_rows is None:
            raise RuntimeError("%s: the tables have no first-order weights (call attach_linear first)" % what)

    def _units1(self, what):
        if self.U > 1:
            raise NotImplementedError("%s: the first-order term over bags carries units = 1 only (the rows hold %d)" % (what, self.U))

    def linear_weights(self):
        """This rank's first-order weights, one [local rows] VIEW of the packed rows per slot ([local rows, U] with units = U > 1)."""
        self._need_linear("linear_weights")
        return [r[:, 0] if self.U == 1 else r[:, 0::4] for r in self.lin_rows]

    def linear_state(self):
        """(w, n, z): per slot the [local rows] views ([local rows, U] with units = U > 1) of the weights and of their FTRL accumulator
        and linear slots."""
        self._need_linear("linear_state")
        return tuple([r[:, c] if self.U == 1 else r[:, c::4] for r in self.lin_rows] for c in range(3))

    def enable_linear_training(self, lr, l1=0.0, l2=0.0):
        """Attach the owner-side FTRL-Proximal of the first-order rows (the reference's linear_optimizer='Ftrl', deepFM.py:58, applied by
        the parameter server that holds the partition): lookup_train(ids, with_linear=True) then also returns the linear term, and its
        backward takes one synchronous FTRL step over the global batch on every rank's rows.  The accumulators' initial value was fixed when
        the rows were packed (attach_linear)."""
        self._need_linear("enable_linear_training")
        if not lr > 0 or l1 < 0 or l2 < 0:
            raise ValueError("enable_linear_training: lr > 0, l1 >= 0, l2 >= 0")
        self._lin_hp = (float(lr), float(l1), float(l2))
        return self

    def _collective(self):
        return self.P > 1 or (self.force_collective and dist.is_initialized())

    def _C(self):
        """Micro-batches per lookup: a constructor constant (never a function of the local batch: every rank issues the same
        number of collectives)."""
        return self.chunks if self._collective() else 1

    def _a2a_staged(self, out, inp, out_splits=None, in_splits=None):
        o = torch.empty(out.shape, dtype=out.dtype)
        dist.all_to_all_single(o, inp.cpu(), out_splits, in_splits, group=self.group)
        out.copy_(o)

    def _a2a(self, out, inp, out_splits, in_splits):
        if not self._collective():
            out.copy_(inp)
        elif _host_staged(out, self.group):
            self._a2a_staged(out, inp, out_splits, in_splits)
        else:
            dist.all_to_all_single(out, inp, out_splits, in_splits, group=self.group)

    def _a2a_equal(self, out, inp):
        """Equal-split all-to-all, asynchronous where the transport allows: -> a work handle (or None when done / aliased)."""
        if not self._collective():
            return None                                   # out IS inp (see _Plan)
        if _host_staged(out, self.group):
            return self._a2a_staged(out, inp)
        return dist.all_to_all_single(out, inp, group=self.group, async_op=True)

    def _max_over_ranks(self, values):
        """MAX over the ranks of a few host integers (a capacity agreement): on the host for gloo, through the device otherwise."""
        t = torch.tensor(values, dtype=torch.int64)
        if dist.get_backend(self.group) == "gloo":
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        else:
            td = t.to(self.device)
            dist.all_reduce(td, op=dist.ReduceOp.MAX, group=self.group)
            t = td.cpu()
        return [int(v) for v in t]

    # ---- the steps that have a grouped form: today's backend call at G = 1, the grouped one otherwise ----------------------
    def _new_out(self, B, device):
        """The result buffer(s) of a lookup: [B, F*K], or a tuple of G of them over row groups."""
        if self.G == 1:
            return torch.empty((B, self.F * self.K), dtype=torch.float32, device=device)
        return tuple(torch.empty((B, self.F * self.K), dtype=torch.float32, device=device) for _ in range(self.G))

    def _finish_groups(self, back, inv2d, out, s=None, e=None):
        """Row groups: the finish pass of samples [s, e) (None: all) from `back` through inv2d into the G outputs.  -> (out, None)"""
        self.backend.finish_groups(back, inv2d, self.K, list(out) if s is None else [o[s:e] for o in out])
        return out, None

    # ---- training: the gradient rows travel the forward's row exchange backwards and the OWNER updates its shard -------
    def enable_training(self, lr, initial_accumulator_value=0.1):
        """Attach the owner-side sparse Adagrad (the reference's dnn_optimizer='Adagrad', deepFM.py:61, applied by the
        parameter server that holds the partition: deepFM.py:163-167).  lookup_train() then returns an embedding matrix
        whose backward() updates every rank's shard in place; duplicate rows -- from one rank or several -- are summed
        first, i.e. one synchronous step over the global batch."""
        self.optimizer = self.backend.make_optimizer(lr, initial_accumulator_value)
        self._adam = False
        return self

    def enable_training_adam(self, beta1=0.9, beta2=0.999, eps=1e-8, clip_norm=0.0):
        """Attach the owner-side sparse Adam instead (the reference DCN's train_op on its embedding variables: tf.train.AdamOptimizer with
        tf.clip_by_norm(g, 100) per variable, DeepCrossNetwork.py:264-290).  Every rank holds m and v (zeros) of its
        shards; lookup_train(ids).backward() then takes one synchronous [TF-upstream] sparse Adam step over the global batch:
          1. the gradient rows travel the forward's row exchange backwards, as for Adagrad;
          2. every owner sorts what it received and adds up its rows' share of each table's ||g||^2 (fixed point, integer adds);
          3. the shares are summed over the ranks -- an exact integer sum, the same on every rank, whatever P and the arrival order --
             because tf.clip_by_norm divides by the norm of the WHOLE table's gradient;
          4. every owner steps its touched rows with the global norms, then decays and steps every other local row: TF's sparse Adam moves
             every row every step, so an owner that received nothing still takes part in 3 and still runs 4.
        clip_norm == 0: no clip, so no norm pass and no collective.  Set `tables.optimizer.lr_t` (lr * sqrt(1 - beta2^t) / (1 - beta1^t), t
        = the ONE global step + 1, the same on every rank) before every backward -- ShardedDCNTrainer's train_spec.TrainStep does.
        lookup_bags_train(...).backward() takes the same step over the bag records the owners kept (section 5.3: a row's summed record
        gradient goes through the slot's max_norm clip derivative first, and that is the gradient whose norm is taken) on a backend
        with bags_adam_norm / bags_adam_apply; one-hot and bag steps may alternate.
        Not covered (each raises): with_linear=True, row groups, graph capture of a step."""
        if self.G > 1:
            raise NotImplementedError("enable_training_adam: row groups (groups=%d) are trained with the owner-side Adagrad only" % self.G)
        if not all(hasattr(self.backend, n) for n in ("make_adam", "adam_norm", "adam_apply")):
            raise NotImplementedError("enable_training_adam: this backend has no owner-side Adam (make_adam / adam_norm / adam_apply)")
        if not (0 <= beta1 < 1 and 0 <= beta2 < 1 and eps > 0 and clip_norm >= 0):
            raise ValueError("enable_training_adam: 0 <= beta < 1, eps > 0, clip_norm >= 0")
        self.optimizer = self.backend.make_adam(float(beta1), float(beta2), float(eps), float(clip_norm))
        self._adam = True
        self._adam_clip = float(clip_norm)
        return self

    def adam_state(self):
        """(m, v): per slot this rank's [local rows, K] first and second moments (enable_training_adam first)."""
        if not self._adam:
            raise RuntimeError("call enable_training_adam() first")
        return self.optimizer.ms, self.optimizer.vs

    def _sum_norm_shares(self, share):
        """share [2, F] int64: this owner's norm words (ops.SparseAdam.norm_payload: row 0 the low word, < 2^32, in units of 2^-32; row 1
        the high word, the integer part) -> [F] float64, every table's GLOBAL ||g||^2 in plain units, the same value on every rank.  The
        two rows are summed over the ranks as int64 vectors (64 ranks x 2^32 cannot wrap the low row; the high row holds while the global
        ||g||^2 stays below 2^62) and recombined in double: an exact integer sum -- independent of P and of the order the shares arrive
        in -- rounded once.  On the host for gloo, through the device otherwise (as _max_over_ranks).
        A backend may still hand over ONE word per table (share [F]: the bits of a u64 in 2^-32 fixed point, good below ||g||^2 = 2^32 on
        that owner): it is read as its 32-bit halves, the same two rows."""
        if share.dim() == 1:
            share = torch.stack([share & 0xffffffff, (share >> 32) & 0xffffffff])
        halves = torch.stack([share[1], share[0]])
        if self._collective():
            if dist.get_backend(self.group) == "gloo":
                h = halves.cpu()
                dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.group)
                halves = h.to(share.device)
            else:
                dist.all_reduce(halves, op=dist.ReduceOp.SUM, group=self.group)
        high = halves[0] + (halves[1] >> 32)               # the carry of the summed low words: both terms below are exact doubles
        return high.double() + (halves[1] & 0xffffffff).double() / 4294967296.0

    def _refuse_adam_capture(self, t):
        if self._adam and t.is_cuda and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("a sharded Adam step cannot be captured in a graph (its norm exchange is a collective between the two "
                                      "halves of the owner's step)")

    def _owner_step(self, payload, grad_rows):
        """The owner-side step of the embedding rows over (payload, gradient rows) as received from all ranks."""
        be = self.backend
        if not self._adam:
            return be.apply_adagrad(self.optimizer, payload, grad_rows)
        self._refuse_adam_capture(payload)
        norms = None
        if self._adam_clip > 0:          # every rank, also one that received nothing: the sum is a collective
            norms = self._sum_norm_shares(be.adam_norm(self.optimizer, payload, grad_rows))
        be.adam_apply(self.optimizer, payload, grad_rows, norms)

    def _need_dedup_train(self, what, with_linear=False):
        """The combinations de-duplicated training does not cover, refused before anything is enqueued."""
        if with_linear and not hasattr(self.backend, "rows_scatter_sum_side"):
            raise NotImplementedError("%s with with_linear=True: this backend has no scatter-sum with a side sum (rows_scatter_sum_side), and "
                                      "the first-order term's plain backward writes one slab position per entry; train it with dedup=False"
                                      % what)
        if self.G > 1:
            raise NotImplementedError("%s: row groups (groups=%d) are trained one slab position per entry (dedup=False) only" % (what, self.G))
        if with_linear and self.U != 1:
            raise NotImplementedError("%s with with_linear=True: one first-order unit per row only (units=%d)" % (what, self.U))
        if not hasattr(self.backend, "rows_scatter_sum"):
            raise NotImplementedError("%s: this backend has no scatter-sum of gradient rows (rows_scatter_sum)" % what)

    def lookup_train(self, ids, with_linear=False, dedup=False):
        """Differentiable lookup: emb [B_local, F*K] with a grad_fn (the tables themselves get no .grad).  Runs the fixed-capacity
        pipeline (no split sizes reach the host; the gradient rows go back through the same equal-split slabs); the exact
        variable-size path only when mode == "exact", after an overflow, or when "auto" has given up on slabs.  One training lookup
        may be outstanding (forward -> backward) per ShardedTables.
        with_linear: -> (emb, lin) from ONE autograd node; lin [B_local, 1] = the sum of the sample's F first-order weights (no bias: the
        bias is a replicated dense variable of the caller's).  Its backward receives both gradients: the row gradients and d lin travel
        the same equal-split exchange, then every owner applies Adagrad to its embedding rows and FTRL to its first-order rows (in that
        order: the FTRL step reuses the Adagrad step's sort of the payload) -- one optimiser step.
        dedup: the training exchange sends each distinct (slot, row) of a 2048/4096-sample tile once (the de-duplicating bucket kernel, on
        a capacity and plans of its own); the backward sums the gradients of the entries that share a slab position on the requester
        (backend.rows_scatter_sum: sorted, compensated, no float atomics) before the reversed exchange, and the owner -- which sees fewer
        payload words -- still sums duplicates across tiles, micro-batches and ranks.  The forward is bit for bit dedup=False's.  The
        exact path (mode="exact", overflow repair) stays one row per entry.  with_linear=True under dedup: d lin is summed per slab
        position by the SAME call on the same sort (backend.rows_scatter_sum_side: one call per micro-batch gives the gradient slab and
        the first-order slab), and the owner's FTRL sums what is left across tiles, micro-batches and ranks before its non-linear rule.
        Not covered (each raises NotImplementedError): row groups, a backend without rows_scatter_sum (with_linear: without
        rows_scatter_sum_side)."""
        if self.optimizer is None:
            raise RuntimeError("call enable_training(lr) first")
        if dedup:
            self._need_dedup_train("lookup_train(dedup=True)", with_linear)
        self._refuse_adam_capture(ids)                   # before anything is enqueued, not first inside backward()
        if with_linear and self._adam:
            raise NotImplementedError("lookup_train(with_linear=True) under enable_training_adam: the first-order rows' FTRL rides on the Adagrad "
                                      "step's sort only")
        if with_linear:
            self._need_linear("lookup_train(with_linear=True)")
            if self._lin_hp is None:
                raise RuntimeError("call enable_linear_training(lr) first")
        anchor = torch.zeros((), dtype=torch.float32, device=ids.device, requires_grad=True)
        res = _ShardedLookup.apply(self, ids, bool(with_linear), anchor, bool(dedup))
        if self.G == 1:
            return res
        # row groups: a tuple of G embedding matrices (one autograd node: their gradients go back interleaved in ONE row exchange and
        # the owner takes ONE Adagrad step at width G*K), or (that tuple, lin [B_local, U])
        return (tuple(res[:self.G]), res[self.G]) if with_linear else tuple(res)

    def lookup_rows_train(self, ids, dedup=True):
        """The training lookup WITHOUT its finish pass (what lookup_rows is to lookup): -> a handle with
          .rows [R, K]: the received rows of ALL micro-batches as one matrix (chunk c's slab positions offset by c * P * cap), private to
                 the training plans -- an inference lookup between this call and backward_rows leaves them alone;
          .inv  [B_local, F] int64: the position of every entry's row in .rows, < 0 where the id was pruned / out of range;
          .backward_rows(idx, grad_rows): the per-position sum of the gradient rows (any number of entries per position, any order),
                 the reversed exchange and the owner's step.  Exactly once.
        A model whose kernels take (table, ids) trains with table = .rows (a leaf that requires grad) and ids = .inv; the sparse gradient
        it leaves on that leaf is (idx, grad_rows).  dedup (the default): each distinct (slot, row) of a tile is sent once, on the
        de-duplicated training capacity (lookup_train(dedup=True)'s).  The overflow verdict is read here, once, as lookup_train does; an
        overflow is repaired on the exact path (.rows then holds one row per entry).  One training lookup may be outstanding per
        ShardedTables; every rank must call it (SPMD)."""
        if self.optimizer is None:
            raise RuntimeError("call enable_training(lr) first")
        self._need_dedup_train("lookup_rows_train")
        self._refuse_adam_capture(ids)
        if ids.dim() != 2 or ids.shape[1] != self.F:
            raise ValueError("ids must be [B, F=%d]" % self.F)
        (rows, inv), saved, _ = self._forward_train(ids, False, dedup=bool(dedup), rows_only=True)
        return _RowsTrainLookup(self, saved, rows, inv)

    def _forward_train(self, ids, with_lin, dedup=False, rows_only=False):
        """The forward of a training lookup -> (emb, what the backward needs, lin [B, 1] | None).  On the fixed-capacity pipeline (one slab
        position per entry; dedup: one per distinct row of a tile, on the de-duplicated training capacity and plans) unless mode == "exact",
        "auto" has given up on slabs, or a slab overflows.  rows_only (lookup_rows_train): no finish pass -- emb is (rows [R, K], inv [B, F]),
        the received rows of all micro-batches as one matrix and every entry's position in it (< 0: pruned).  The overflow verdict is read here (the one host wait of a training lookup; it covers work that is long done when
        the dense part of the model has been enqueued in between); the exact path keeps a row buffer of its own."""
        B, F = ids.shape
        lin = (torch.empty((B, self.U), dtype=torch.float32, device=ids.device), None) if with_lin else None
        if not (self._use_exact or B == 0 and not self._collective()):
            out = None if rows_only else self._new_out(B, ids.device)
            plan = self._plan(B, "train_dedup" if dedup else "train")
            done = self._enqueue(plan, ids, False, out, None, dedup=bool(dedup), lin=lin, consumer=(lambda s, e, rows, inv: None) if rows_only else None)
            _Lookup(self, plan, ids, False, out, None, done).join()
            over = False
            if done is not False:
                over, demand = self._read_flags(plan, done)
                self._learn(plan, over, demand)
            if not over:
                if rows_only:
                    out = (plan.back_all, self._rows_inv(plan, F, ids.device))
                return out, ("fixed", plan), lin[0] if with_lin else None
            self.stats["fallbacks"] += 1
        back, inv, sc, rc, recv = self._exchange_exact(ids, lin, private=True)
        if rows_only:
            # (the exact path gives pruned entries a position too -- a zero row; the handle's contract is inv < 0 there)
            live = (ids >= 0) & (ids < self.vocab_dev.unsqueeze(0))
            return (back, torch.where(live, inv.view(B, F), torch.full_like(ids, -1))), ("exact", inv, sc, rc, recv, True), None
        if dedup:                                        # (one row per entry here: the backward's scatter-sum sees only runs of one)
            emb, _ = self.backend.finish(back, inv, B, F, False)
            return emb, ("exact", inv, sc, rc, recv, True), lin[0] if with_lin else None
        if self.G == 1:
            emb, _ = self.backend.finish(back, inv, B, F, False)
        else:
            emb, _ = self._finish_groups(back, inv.view(B, F), self._new_out(B, ids.device))
        return emb, ("exact", inv, sc, rc, recv), lin[0] if with_lin else None

    def _rows_inv(self, plan, F, device):
        """[B, F] int64: every entry's position in plan.back_all (chunk c's slab positions offset by c * P * cap), < 0 where pruned."""
        be, span = self.backend, self.P * plan.cap
        parts = []
        for c, (s, e) in enumerate(plan.bounds):
            if e > s:
                iv = be.inv2d(plan.inv[c], e - s, F, plan.dedup)
                parts.append(torch.where(iv < 0, iv, iv + c * span) if c else iv)
        if not parts:
            return torch.empty((0, F), dtype=torch.int64, device=device)
        return (parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)).contiguous()

    def _linear_exact(self, recv, inv2d, sc, rc, lin):
        """The linear term on the exact path: one weight per received payload word, sent back with the row exchange's splits (one float
        per entry), summed per sample."""
        U = self.U                                       # floats per entry
        n = inv2d.numel()
        lw = torch.empty(recv.numel() * U, dtype=torch.float32, device=recv.device)
        self.backend.linear_gather(recv, None, lw)
        lback = torch.empty(n * U, dtype=torch.float32, device=recv.device)
        self._a2a(lback, lw, [c * U for c in sc], [c * U for c in rc])
        self.backend.linear_finish(lback, inv2d, lin[1], lin[0])

    def _backward_apply(self, saved, g_emb, g_lin=None, slabs=None):
        """g_lin (lookup_train(with_linear=True)): d loss / d lin [B_local, 1].  Its values go where the weights came back from and travel
        the same exchange as the gradient rows; the owner's FTRL runs after its Adagrad, over the same payload, on that step's sort.
        The exchange is the same under enable_training_adam; the owner's step (_owner_step) is then norm pass, norm sum over the ranks, apply.
        slabs (lookup_rows_train's backward_rows; g_emb is None): the gradient slabs already built -- [C * P * cap, K] on the fixed path,
        [n, K] in exchange order on the exact path."""
        K, G = self.K, self.G
        be = self.backend
        U = self.U
        self._updates += 1
        if G > 1:                                        # row groups: g_emb = the G gradients; they travel interleaved, G*K floats per position
            gs = [g.contiguous() for g in g_emb]
            dev = gs[0].device
        if saved[0] == "fixed":
            plan = saved[1]
            P, cap = self.P, plan.cap
            C = plan.C
            g2 = g_emb.contiguous() if G == 1 and slabs is None else None
            works, grecv_l = [], []
            for c, (s, e) in enumerate(plan.bounds):
                # entry i's gradient row goes to slab position inv[i] (row P*cap = a dump row for pruned entries); owners receive
                # the slabs through the forward row exchange reversed (equal splits again)
                if slabs is not None:
                    gsend = slabs[c * P * cap:(c + 1) * P * cap]
                elif plan.dedup:
                    # de-duplicated: many entries share a position -- their rows are summed in entry order (sorted, compensated, no
                    # atomics); positions nobody names come out as zeros
                    gsend = torch.empty((P * cap, K), dtype=torch.float32, device=g2.device)
                    idx = be.inv2d(plan.inv[c], e - s, self.F, True).reshape(-1)
                    if g_lin is None:
                        be.rows_scatter_sum(idx, g2[s:e].reshape(-1, K), P * cap, gsend)
                    else:
                        # ... and d lin with them, on the same sort: entry i belongs to sample i // F, so g_lin is read in place and the
                        # first-order slab (this micro-batch's lrows) comes out of the same call
                        be.rows_scatter_sum_side(idx, g2[s:e].reshape(-1, K), g_lin[s:e], self.F, P * cap, gsend,
                                                 plan.lin_buffers(U)[0][c].view(P * cap, U))
                elif G > 1:
                    # ... by the HIP transpose of the grouped finish: zero-fill + one writer per position, no dump row
                    gsend = torch.empty((P * cap, self.KW), dtype=torch.float32, device=dev)
                    be.grad_groups([g[s:e] for g in gs], be.inv2d(plan.inv[c], e - s, self.F, False), K, gsend)
                else:
                    gsend = torch.zeros((P * cap + 1, K), dtype=torch.float32, device=g2.device)
                    if e > s:
                        inv = plan.inv[c]
                        idx = torch.where(inv < 0, torch.full_like(inv, P * cap), inv)
                        gsend.index_copy_(0, idx, g2[s:e].reshape(-1, K))
                    gsend = gsend[:P * cap]
                grecv = gsend
                if self._collective():
                    grecv = torch.empty((P * cap, self.KW), dtype=torch.float32, device=gsend.device)
                    self._a2a(grecv.view(-1), gsend.reshape(-1), None, None)
                grecv_l.append(grecv)
                if g_lin is not None:
                    # the forward's linear buffers carry the gradient back: lrows = what this rank sends, lback = what it receives
                    lrows, lback = plan.lin_buffers(U)
                    if not plan.dedup:                   # (de-duplicated: rows_scatter_sum_side has written lrows[c] above)
                        be.linear_grad(g_lin[s:e], be.inv2d(plan.inv[c], e - s, self.F, False), lrows[c])
                    if self._collective():
                        self._a2a(lback[c], lrows[c], None, None)
            # ONE update over all micro-batches (duplicates of a row -- from any chunk, any rank -- are summed before the accumulator
            # moves: a synchronous step over the global batch)
            slabs = plan.recv_all.view(C * P, cap + 1)
            hdr = slabs[:, 0] & 0xffffffff
            pos = torch.arange(cap, device=slabs.device)
            pay = torch.where(pos.unsqueeze(0) < hdr.unsqueeze(1), slabs[:, 1:], torch.full_like(slabs[:, 1:], -1)).reshape(-1)
            self._owner_step(pay, grecv_l[0] if C == 1 else torch.cat(grecv_l, dim=0))
            if g_lin is not None:
                be.apply_ftrl(pay, plan.lback_all.view(-1), *self._lin_hp, sorted_by=self.optimizer)
            return
        _, inv, sc, rc, recv = saved[:5]
        n = inv.numel()
        KW = self.KW
        if slabs is not None:
            gsend = slabs
        elif len(saved) > 5 and saved[5]:                # a de-duplicated lookup repaired on the exact path: the same kernel, runs of one
            gsend = torch.empty((n, K), dtype=torch.float32, device=g_emb.device)
            be.rows_scatter_sum(inv, g_emb.contiguous().view(n, K), n, gsend)
        elif G == 1:
            g = g_emb.contiguous().view(n, K)
            gsend = torch.empty_like(g)
            gsend[inv] = g                               # entry e's row sits at position inv[e] of the exchange order
        else:
            gsend = torch.empty((n, KW), dtype=torch.float32, device=dev)
            be.grad_groups(gs, inv.view(-1, self.F), K, gsend)
        dev = gsend.device
        grecv = torch.empty((recv.numel(), KW), dtype=torch.float32, device=dev)
        self._a2a(grecv.view(-1), gsend.view(-1), [c * KW for c in rc], [c * KW for c in sc])   # the forward exchange, reversed
        self._owner_step(recv, grecv)
        if g_lin is not None:
            lsend = torch.empty(n * U, dtype=torch.float32, device=dev)
            be.linear_grad(g_lin, inv.view(-1, self.F), lsend)
            lrecv = torch.empty(recv.numel() * U, dtype=torch.float32, device=dev)
            self._a2a(lrecv, lsend, [c * U for c in rc], [c * U for c in sc])
            be.apply_ftrl(recv, lrecv, *self._lin_hp, sorted_by=self.optimizer)

    # ---- the exact, variable-size lookup (one host read of the split sizes) --------------------------------
    def _exchange_exact(self, ids, lin=None, private=False):
        """Bucket, exchange the ids, gather on the owner, exchange the rows (and the linear term behind them).  -> (back [n, K]: the rows
        in exchange order, inv [n]: every entry's position in it, send counts, receive counts, the payload received).
        private: a fresh row buffer instead of the backend's cached one (training: an inference lookup between a forward and its backward
        must not touch it)."""
        B, F = ids.shape
        K, be = self.KW, self.backend
        flat = ids.reshape(-1).contiguous()
        n = flat.numel()
        payload, inv, send_counts, _ = be.bucket(flat)                      # HIP
        recv_counts = torch.empty_like(send_counts)
        self._a2a(recv_counts, send_counts, None, None)
        both = torch.stack([send_counts, recv_counts]).tolist()             # the host read of this path
        sc, rc = [int(v) for v in both[0]], [int(v) for v in both[1]]
        recv = torch.empty(sum(rc), dtype=torch.int64, device=flat.device)
        self._a2a(recv, payload, rc, sc)
        rows = be.gather_packed(recv)                                       # HIP (owner side)
        back = torch.empty((n, K), dtype=torch.float32, device=flat.device) if private else be.back_buffer(n, K, flat.device)
        self._a2a(back.view(-1), rows.reshape(-1), [c * K for c in sc], [c * K for c in rc])
        if lin is not None:
            self._linear_exact(recv, inv.view(B, F), sc, rc, lin)
        return back, inv, sc, rc, recv

    def _lookup_exact(self, ids, want_fm, out=None, fm=None, consumer=None, lin=None):
        B, F = ids.shape
        back, inv = self._exchange_exact(ids, lin)[:2]
        if consumer is not None:                                            # (lookup_consume: the caller's kernel reads the rows where they are)
            consumer(0, B, back, inv.view(B, F))
            return None, None
        if self.G > 1:
            return self._finish_groups(back, inv.view(B, F), out if out is not None else self._new_out(B, ids.device))
        return self.backend.finish(back, inv, B, F, want_fm, out=out, fm=fm)    # HIP: un-permute (+ FM)

    # ---- the fixed-capacity, pipelined lookup ---------------------------------------------------------------
    def _default_cap(self, n_chunk):
        P = self.P
        if self.slack is not None:
            return _round_up(max(1, math.ceil(float(self.slack) * n_chunk / P)), 16)
        p = 1.0 / P
        return min(_round_up(n_chunk * p + 8.0 * math.sqrt(n_chunk * p * (1 - p)) + 64, 16), _round_up(max(n_chunk, 16), 16))

    def _agree_cap(self, B):
        """The ONE agreement the equal-split exchanges need, at the first fixed-capacity lookup (every rank's first lookup: SPMD):
        slab capacity = MAX over the ranks of the default for their batch (or max_batch).  Later changes (_learn) are functions of
        numbers every rank reads identically off the slab headers, so no rank ever decides alone."""
        Bm = max(int(B), int(self.max_batch or 0))
        n_chunk = max(1, -(-Bm // self._C())) * self.F
        cap = self._default_cap(n_chunk)
        cap, n_chunk = self._max_over_ranks([cap, n_chunk])
        self._cap = self._cap_train = self._cap_train_dedup = self._cap0 = cap
        self._share0 = float(n_chunk) / self.P            # an owner's share of a micro-batch without skew

    def _plan(self, B, slot=0):
        if self._collective():
            if self._cap is None:
                self._agree_cap(B)
            # two capacities: the plain training pipeline keeps one slab position per entry (dedup=False), so what de-duplicated
            # inference lookups learn (a SMALLER capacity) must not shrink its slabs -- sharing one number made every training lookup
            # after an inference lookup overflow and run twice
            # ... and a third: de-duplicated TRAINING (lookup_train(dedup=True), lookup_rows_train) learns how many distinct rows a
            # micro-batch leaves per owner and shrinks to that -- the link bytes it exists to save.  That number must neither shrink the
            # one-position-per-entry training slabs nor move the inference capacity, and neither of those may grow or shrink it.
            cap = self._cap_of(slot)
        else:
            cap = _round_up(max(B * self.F, 16), 16)      # one rank: a slab holds the whole batch, nothing can overflow
        key = (B, slot, cap)
        plan = self._plans.get(key)
        if plan is None:
            def live(k):      # plans of other (batch, slot) pairs whose slabs still have the capacity in use for their kind
                if (k[0], k[1]) == (B, slot):
                    return False
                return not self._collective() or k[2] == self._cap_of(k[1])
            self._plans = {k: v for k, v in self._plans.items() if live(k)}
            if len(self._plans) > 8:
                self._plans.clear()
            plan = self._plans[key] = _Plan(self, B, cap, train=slot in ("train", "train_dedup"))
            plan.slot, plan.dedup = slot, slot == "train_dedup"
        self.stats["cap"] = cap
        return plan

    def _cap_of(self, slot):
        """The agreed slab capacity the plans of `slot` follow: "train", "train_dedup", or anything else = the inference capacity."""
        return self._cap_train if slot == "train" else self._cap_train_dedup if slot == "train_dedup" else self._cap

    def _ensure_streams(self):
        if self._streams is None and self.device.type == "cuda":
            if self.side_cus:
                self._streams = [_masked_stream(self.device, self.side_cus, k) for k in range(2)]
            else:
                self._streams = [torch.cuda.Stream(device=self.device), torch.cuda.Stream(device=self.device)]
            self._chk_stream = torch.cuda.Stream(device=self.device)
        return self._streams

    def _enqueue(self, plan, ids, want_fm, out, fm, dedup, consumer=None, lin=None):
        """Enqueue one lookup's pipeline.  -> False (nothing to check: one rank, slabs hold the whole batch), None (statistic in
        plan.stat, no event: CPU backend) or the event after which plan.host holds [overflow, demand].
        lin = (lin [B, 1], bias | None): the first-order term rides along -- per micro-batch the owner reads one weight per received
        slab slot right after the row gather, one float per slot goes back behind the rows, and the requester sums its samples' weights
        beside the finish pass; without it nothing here changes."""
        B, F = ids.shape
        be, P = self.backend, self.P
        C = plan.C
        cap = plan.cap
        lrows, lback = plan.lin_buffers(self.U) if lin is not None else (None, None)
        if not self._collective():
            # one rank, no exchange: the three kernels back to back on the caller's stream
            be.bucket_cap(ids, cap, plan.send[0], plan.inv[0], plan.counts[0], plan.flags[0], plan.ws[0], stat=plan.cstat[0], dedup=dedup)
            be.gather_slabs(plan.recv[0], cap, plan.rows[0])
            if lin is not None:
                be.linear_gather(plan.recv[0], cap, lrows[0])
                if B:
                    be.linear_finish(lback[0], be.inv2d(plan.inv[0], B, F, dedup), lin[1], lin[0])
            if B and consumer is not None:
                consumer(0, B, plan.back[0], be.inv2d(plan.inv[0], B, F, dedup))
            elif B and self.G > 1:
                self._finish_groups(plan.back[0], be.inv2d(plan.inv[0], B, F, dedup), out)
            elif B:
                be.finish_chunk(plan.back[0], be.inv2d(plan.inv[0], B, F, dedup), want_fm, out, fm if want_fm else None)
            return False
        S = self._ensure_streams()
        cur = torch.cuda.current_stream(self.device) if S else None
        if S:
            for s in S:
                s.wait_stream(cur)

        def on(c):
            return torch.cuda.stream(S[c % 2]) if S else contextlib.nullcontext()

        def bucket(c):
            s, e = plan.bounds[c]
            be.bucket_cap(ids[s:e], cap, plan.send[c], plan.inv[c], plan.counts[c], plan.flags[c], plan.ws[c], stat=plan.cstat[c], dedup=dedup)
            return self._a2a_equal(plan.recv[c], plan.send[c])

        def finish(c):
            s, e = plan.bounds[c]
            if lin is not None:
                _wait(wl[c])
                if e > s:
                    be.linear_finish(lback[c], be.inv2d(plan.inv[c], e - s, F, dedup), lin[1], lin[0][s:e])
            if e > s and consumer is not None:
                consumer(s, e, plan.back[c], be.inv2d(plan.inv[c], e - s, F, dedup))
            elif e > s and self.G > 1:
                self._finish_groups(plan.back[c], be.inv2d(plan.inv[c], e - s, F, dedup), out, s, e)
            elif e > s:
                be.finish_chunk(plan.back[c], be.inv2d(plan.inv[c], e - s, F, dedup), want_fm, out[s:e], fm[s:e] if want_fm else None)

        wi, wr, wl = [None] * C, [None] * C, [None] * C
        ev_ids = []
        with on(0):
            wi[0] = bucket(0)
        for c in range(C):
            if c + 1 < C:
                with on(c + 1):
                    wi[c + 1] = bucket(c + 1)
            with on(c):
                _wait(wi[c])
                if S:
                    ev_ids.append(S[c % 2].record_event())
                be.gather_slabs(plan.recv[c], cap, plan.rows[c])
                wr[c] = self._a2a_equal(plan.back[c], plan.rows[c])
                if lin is not None:
                    be.linear_gather(plan.recv[c], cap, lrows[c])
                    wl[c] = self._a2a_equal(lback[c], lrows[c])
            if c >= 1:
                with on(c - 1):
                    _wait(wr[c - 1])
                    finish(c - 1)
        # every micro-batch's slabs have arrived: their headers carry every sender's demand -> the verdict all ranks agree on
        done = None
        ctx = torch.cuda.stream(self._chk_stream) if S else contextlib.nullcontext()
        with ctx:
            if S:
                for e in ev_ids:
                    self._chk_stream.wait_event(e)
            be.slab_stat(plan.recv_all, C * P, cap, plan.stat)
            if S:
                plan.host.copy_(plan.stat, non_blocking=True)
                done = self._chk_stream.record_event()
        with on(C - 1):
            _wait(wr[C - 1])
            finish(C - 1)
        plan.fin = [s.record_event() for s in S] if S else None
        return done

    def _read_flags(self, plan, done):
        """The overflow verdict and the largest demand of a lookup, identical on every rank.  On the GPU the header scan and its copy
        to pinned memory ran on their own stream right behind the LAST id exchange: the host waits for work that is long done while
        the row exchanges and finish kernels keep the GPU busy."""
        if done is not None:
            done.synchronize()
            host = plan.host
        else:
            host = plan.stat.cpu()
        return bool(host[0]), int(host[1])

    def _learn(self, plan, over, demand):
        """Capacity policy after a checked lookup (inputs identical on every rank): grow to the observed demand after an overflow;
        with dedup, shrink to what de-duplication left; give up on fixed slabs (mode auto) when one owner wants more than twice
        the no-skew share -- padding every slab to that size would cost more link bytes than the exact path's host read."""
        train = plan.train
        if plan.cap != self._cap_of(plan.slot):
            return                                         # a verdict about slabs that are no longer in use
        cap = plan.cap
        if over:
            cap = max(cap, _round_up(demand * 1.25 + 64, 16))
        elif plan.dedup if train else self.dedup:          # only verdicts of de-duplicated lookups say what de-duplication left
            want = _round_up(demand * 1.25 + 64, 16)
            if want < 0.7 * cap:
                cap = want
        if plan.dedup:
            self._cap_train_dedup = cap
        elif train:
            self._cap_train = cap
        else:
            self._cap = cap
        if self.mode == "auto" and demand > 2.0 * self._share0 + 16:
            self._use_exact = True

    def _drain_unchecked(self, block):
        keep = []
        for lk in self._unchecked:
            if lk.checked:
                continue
            if not block and lk.done is not None and not lk.done.query():
                keep.append(lk)
                continue
            lk.checked = True
            over, demand = self._read_flags(lk.plan, lk.done)
            self._learn(lk.plan, over, demand)
            if over:
                self._unchecked = keep
                raise RuntimeError("ShardedTables: a slab of an earlier fixed-capacity lookup overflowed (demand %d > capacity %d): "
                                   "that result was incomplete" % (demand, lk.plan.cap))
        self._unchecked = keep

    def check_overflow(self):
        """check="lazy"/"never": read the verdicts of the fixed-capacity lookups (and lookup_bags calls) not checked yet; raises if a slab
        overflowed (that result was incomplete: repeat it with mode="exact" or a larger slack; the bag capacities have grown already)."""
        self._drain_bag_unchecked()
        self._drain_unchecked(block=True)
        return False

    def lookup_async(self, ids, want_fm=False, out=None, fm=None, consumer=None, want_lin=False, lin=None, lin_bias=None):
        """Enqueue a lookup and return a handle; handle.result() -> emb [B_local, F*K] (or (emb, fm)).  Two lookups can be in
        flight (double-buffered plans): issue lookup i+1, then consume lookup i -- the exchange of i+1 runs under that compute.
        consumer: see lookup_consume (no emb / fm are produced then).
        want_lin: the result carries the first-order term as its last element -- (emb, lin) or (emb, fm, lin), emb = None under a
        consumer; lin [B_local, 1] = the sum of the sample's F first-order weights (attach_linear) + lin_bias (a [1] device tensor, or
        None), ops.linear_logit's over the unsharded packed rows bit for bit.  lin: a preallocated result."""
        B, F = ids.shape
        if F != self.F:
            raise ValueError("ids must be [B, F=%d]" % self.F)
        if self.G > 1:                # (before anything is launched)
            if want_fm:
                self._no_groups("want_fm (the FM term)")
            if consumer is not None:
                self._no_groups("lookup_consume / lookup_rows (a lookup without its finish pass)")
            if out is not None and (len(out) != self.G or any(o.shape != (B, F * self.K) for o in out)):
                raise ValueError("out: %d tensors [B, F*K], one per group" % self.G)
        self.stats["lookups"] += 1
        lt = None
        if want_lin:
            self._need_linear("lookup(want_lin=True)")
            lt = (lin if lin is not None else torch.empty((B, self.U), dtype=torch.float32, device=ids.device), lin_bias)
        if self._use_exact or (B == 0 and not self._collective()):
            emb, fmo = self._lookup_exact(ids, want_fm, out=out, fm=fm, consumer=consumer, lin=lt)
            return _Lookup(self, None, ids, want_fm, emb, fmo, None, consumer=consumer, lin=lt)
        if out is None and consumer is None:
            out = self._new_out(B, ids.device)
        if want_fm and fm is None:
            fm = torch.empty((B, 1), dtype=torch.float32, device=ids.device)
        slot = self._slot
        self._slot ^= 1
        prev = self._inflight.get(slot)
        if prev is not None:
            prev.join()                                   # its buffers are about to be reused
        plan = self._plan(B, slot)
        done = self._enqueue(plan, ids, want_fm, out, fm, dedup=self.dedup, consumer=consumer, lin=lt)
        lk = _Lookup(self, plan, ids, want_fm, out, fm, done, consumer=consumer, lin=lt)
        if done is False:
            lk.joined = True                              # ran on the caller's stream
        self._inflight[slot] = lk
        if not lk.checked and self.check != "eager":
            # lazy: the verdicts of the EARLIER lookups are read now, after this one has been enqueued (their header scans finished
            # long ago: the host does not wait and the streams never drain); never: they wait for check_overflow()
            if self.check == "lazy":
                self._drain_unchecked(block=True)
            else:
                self._unchecked = self._unchecked[-1:]    # "never": a plan slot's verdict is overwritten two lookups later -- keep the
            self._unchecked.append(lk)                   # two newest handles only (check_overflow() reads what is still there)
        return lk

    STAGES = ("bucket", "a2a_ids", "owner_gather", "a2a_rows", "finish")

    def stage_times(self, ids, want_fm=True, iters=5):
        """Diagnostic: the fixed-capacity pipeline of ONE lookup with its five stages run back to back on the caller's stream and a
        HIP event between them (the product path, _enqueue, overlaps the chunks on two side streams; here nothing overlaps, so the
        stages add up to MORE than a pipelined lookup costs).  -> ({stage: microseconds}, emb, fm): per stage the sum over the
        lookup's chunks, median over `iters` runs after one warm-up run, on THIS rank (a collective's time includes waiting for the
        slowest peer to arrive).  Every rank must call it (the exchanges are collectives).  The results of the last run are returned
        so that the caller can check them."""
        import time
        self._no_groups("stage_times")
        B, F = ids.shape
        if F != self.F:
            raise ValueError("ids must be [B, F=%d]" % self.F)
        be, cuda = self.backend, self.device.type == "cuda"
        plan = self._plan(B, "stages")
        cap = plan.cap
        out = torch.empty((B, F * self.K), dtype=torch.float32, device=ids.device)
        fm = torch.empty((B, 1), dtype=torch.float32, device=ids.device) if want_fm else None
        runs = []

        def mark():
            if cuda:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                return e
            return time.perf_counter()

        for it in range(iters + 1):
            marks = []
            for c, (s, e) in enumerate(plan.bounds):
                m = [mark()]
                be.bucket_cap(ids[s:e], cap, plan.send[c], plan.inv[c], plan.counts[c], plan.flags[c], plan.ws[c], stat=plan.cstat[c], dedup=self.dedup)
                m.append(mark())
                _wait(self._a2a_equal(plan.recv[c], plan.send[c]))
                m.append(mark())
                be.gather_slabs(plan.recv[c], cap, plan.rows[c])
                m.append(mark())
                _wait(self._a2a_equal(plan.back[c], plan.rows[c]))
                m.append(mark())
                if e > s:
                    be.finish_chunk(plan.back[c], be.inv2d(plan.inv[c], e - s, F, self.dedup), want_fm, out[s:e], fm[s:e] if want_fm else None)
                m.append(mark())
                marks.append(m)
            if cuda:
                torch.cuda.synchronize(self.device)
            if it:
                runs.append([sum((m[k].elapsed_time(m[k + 1]) * 1e3 if cuda else (m[k + 1] - m[k]) * 1e6) for m in marks) for k in range(5)])
        runs.sort(key=lambda r: sum(r))
        med = runs[len(runs) // 2]
        return dict(zip(self.STAGES, med)), out, fm

    def absmax(self, every=32):
        """The largest |value| over ALL ranks' slices of the tables: the local TableSet.absmax(), then a MAX all-reduce.  WHETHER the
        collective runs is decided from rank-invariant state only -- no cached figure yet, `every` owner-side updates since the last one
        (_backward_apply counts them: every rank applies every step, SPMD), or an ops.invalidate_caches() -- never from a rank-local
        float (the ranks used to compare their re-measured local maxima with the cached ones; sparse updates that left one
        rank's largest row untouched sent that rank past the all-reduce while its peers entered it).  Tables written by any other route
        (a checkpoint loaded into the shards): call ops.invalidate_caches() on every rank."""
        hit = self._absmax_all
        gen = ops._CACHE_GEN[0]
        if hit is not None and hit[0] == gen and (self._updates == hit[1] or (every > 1 and 0 < self._updates - hit[1] < every)):
            return hit[2]
        ts = getattr(self.backend, "ts", None)
        val = float(ts.absmax()) if ts is not None else 0.0
        if self._collective():
            t = torch.tensor([val], dtype=torch.float32, device=self.device)
            if _host_staged(t, self.group):
                t = t.cpu()
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
            val = float(t[0])
        self._absmax_all = (gen, self._updates, val)
        return val

    def lookup_consume(self, ids, consumer):
        """The lookup WITHOUT its finish pass (round 5).  consumer(s, e, rows, inv) is called once per micro-batch (on the stream that
        micro-batch's pipeline runs on) with the received rows of local samples [s, e): rows [n, K] fp32 exactly as the exchange
        left them, inv [e - s, F] int64 = the position of (sample, slot)'s row in `rows`, < 0 where the id was pruned / out of range --
        what the finish pass would gather from.  A consumer that looks its input rows up itself -- ops.tower(gather=(rows_as_tables(rows,
        F), inv, ...)): the DeepFM tower kernel with the FM term, or ops.gather_fm -- reads them there, and the [B, F*K] concatenation is
        never written or read: the rank-local passes of a lookup are bucket + owner gather only.
        On a slab overflow (check="eager") the lookup is repeated on the exact path and the consumer called again for the whole batch:
        its outputs must be plain overwrites.  Returns after the caller's stream has been made to wait for the consumer's kernels."""
        self._no_groups("lookup_consume")
        if self.check != "eager":
            raise ValueError("lookup_consume needs check='eager' (the overflow repair calls the consumer again)")
        self.lookup_async(ids, want_fm=False, consumer=consumer).result()

    def lookup_rows_async(self, ids, want_lin=False, lin_bias=None):
        """Enqueue a lookup WITHOUT its finish pass and hand the received rows to the caller (round 6: what lookup_consume gives a callback,
        as a handle -- so that the NEXT lookup can be issued before this one's rows are consumed, like lookup_async).  handle.result() makes
        the caller's stream wait for the exchange, applies the overflow policy and returns a list of (s, e, rows, inv) -- one entry per
        non-empty micro-batch, samples [s, e) of the local batch: rows [n, K] fp32 exactly as the exchange left them, inv [e - s, F] int64 =
        the position of (sample, slot)'s row in `rows`, < 0 where the id was pruned / out of range.  A kernel that takes (tables, ids) reads
        them as (rows_as_tables(rows, F), inv); ops.cin_stack_gather and ops.tower(gather=) take them directly: the [B, F*K] concatenation
        is never written.  The buffers belong to the lookup's plan slot: valid until the lookup after the next one is enqueued (two slots).
        Needs check='eager' (an overflow is repaired on the exact path before the rows are handed out: then ONE entry for the whole batch)."""
        self._no_groups("lookup_rows")
        if self.check != "eager":
            raise ValueError("lookup_rows needs check='eager' (an overflow is repaired before the rows are handed out)")
        chunks = []      # (want_lin: the handle's .lin holds the first-order term [B, 1] (+ lin_bias) after result())

        def collect(s, e, rows, inv):
            if s == 0:
                chunks.clear()                     # (the repair on the exact path calls again, for the whole batch)
            chunks.append((s, e, rows, inv))
        return _RowsLookup(self.lookup_async(ids, want_fm=False, consumer=collect, want_lin=want_lin, lin_bias=lin_bias), chunks)

    def lookup_rows(self, ids):
        return self.lookup_rows_async(ids).result()

    # ---- multi-hot bags, pooled on the owning rank -----------------------------------------------------------
    def _bag_caps(self, B, nnz):
        """(entry capacity, partial-row capacity) of the bag slabs.  One rank: slabs that hold the whole batch (nothing can overflow, no
        verdict to read).  Several: agreed once, at the first lookup_bags (one host MAX over the ranks' defaults); afterwards changed only
        by verdicts every rank reads identically off the slab headers."""
        if not self._collective():
            # entry capacity rounded up to an eighth of its power of two (<= 12.5 % padding): batches of similar nnz share one plan
            n = max(int(nnz), 16)
            return _round_up(n, max(16, 1 << max(0, n.bit_length() - 4))), _round_up(max(B * self.F, 16), 16)
        if self._bag_cap is None:
            ce = self._default_cap(max(1, nnz))
            cb = min(ce, _round_up(max(B * self.F, 16), 16))           # every partial row has at least one entry
            self._bag_cap = tuple(self._max_over_ranks([ce, cb]))
        return self._bag_cap

    def _bag_plan(self, B, cap_e, cap_b):
        key = (B, cap_e, cap_b)
        plan = self._bag_plans.get(key)
        if plan is None:
            if len(self._bag_plans) >= 4:
                self._bag_plans.clear()
            plan = self._bag_plans[key] = _BagPlan(self, B, cap_e, cap_b)
        # a graph captured now writes these buffers through raw pointers: the capture's hold keeps the plan alive past the clear() above
        return ops.held(plan)

    def _bag_host(self):
        """A pinned 3-word buffer for one lookup_bags verdict: a ring of three, so that the verdicts still unread (at most two) keep theirs."""
        if self._bag_hosts is None:
            self._bag_hosts = [torch.empty(3, dtype=torch.int64, pin_memory=True) for _ in range(3)]
        self._bag_host_i = (self._bag_host_i + 1) % 3
        return self._bag_hosts[self._bag_host_i]

    def _bag_verdict(self, pend):
        """Read one lookup_bags verdict (the same words on every rank) and grow the capacities after an overflow.  -> overflowed?"""
        done, host = pend
        if done is not None:
            done.synchronize()
        over, de, db = (int(v) for v in host.tolist())
        if over:
            self.stats["bag_fallbacks"] = self.stats.get("bag_fallbacks", 0) + 1
            ce, cb = self._bag_cap
            self._bag_cap = (max(ce, _round_up(de * 1.25 + 64, 16)), max(cb, _round_up(db * 1.25 + 64, 16)))
        return over

    def _drain_bag_unchecked(self):
        pend, self._bag_unchecked = self._bag_unchecked, []
        over = [self._bag_verdict(p) for p in pend]
        if any(over):
            raise RuntimeError("ShardedTables: a slab of an earlier lookup_bags overflowed: that result was incomplete (the capacities have "
                               "grown to %s)" % (self._bag_cap,))

    def lookup_bags(self, values, offsets, weights=None, combiner="mean", max_norm=None, field_major=False, flags=0, want_fm=False,
                    want_lin=False, lin_combiner="sum", lin_bias=None):
        """Multi-hot bags over the row-sharded tables, pooled on the owning rank: the sharded form of ops.embedding_bag(values, offsets,
        weights, combiner, field_major, flags, max_norm=) (values [nnz] global row ids, offsets [B_local*F+1], bag (b, f) = b*F+f, or f*B+b
        when field_major; weights [nnz] or None; combiner / max_norm: one value or one per slot).  -> (emb [B_local, F*K], fm [B_local, 1]
        or None).

        Every owner pools the entries of a bag it holds (max_norm clip, w * row summed in entry order) and returns ONE partial row per
        (bag, owner); the requester adds a bag's partials in ascending owner order and applies the combiner.  A bag of L entries brings
        back at most min(L, P) rows instead of L.  With one owner per bag -- world size 1, or all of a bag's live entries on one rank --
        the result is ops.embedding_bag's bit for bit; otherwise the partial sums are added in a different order (fp32 rounding only).
        Both exchanges are equal-split all-to-alls; at world size 1 there are none, nothing can overflow and the lookup can be captured
        in a HIP graph after one eager call.  With several ranks the overflow verdict is read off the received headers (the same words on
        every rank) and the capacities grow to the demands the headers carry; the constructor's `check` decides when: "eager" reads it
        after the whole lookup has been enqueued and repeats an overflowing lookup; "lazy" reads it after the NEXT lookup_bags has been
        enqueued (no host wait on a lookup's own work; an overflow raises there, the result it reports on was incomplete); "never" leaves
        it to check_overflow().  Every rank must call it the same number of times (SPMD).

        want_lin: -> (emb, fm, lin); lin [B_local, 1] = the first-order term over the same bags (attach_linear) + lin_bias (a [1] device
        tensor, or None), ops.linear_logit(values, offsets, weights, combiner=lin_combiner, field_major=) over the unsharded weights.  It
        rides on this lookup: the owner pools the first-order weights of each run beside the embedding rows (w * weight summed in entry
        order), ONE float per partial-row position travels back behind the partial rows, and the requester adds a bag's partials in
        ascending owner order, applies lin_combiner -- the model's one linear_sparse_combiner ("sum" | "mean" | "sqrtn"), independent of
        the per-slot `combiner` -- and sums the sample's F bags in slot order.  With one owner per bag and flags = 0 the result is
        ops.linear_logit's bit for bit.  The term sees the lookup's live entries: under PRUNE_NONPOSITIVE_WEIGHTS the pruned entries
        contribute to neither term.  An overflow repeat carries it; without want_lin nothing here changes."""
        self._no_groups("lookup_bags")
        B = self._bag_args(values, offsets, weights, "lookup_bags")
        lin = None
        if want_lin:
            self._need_linear("lookup_bags(want_lin=True)")
            self._units1("lookup_bags(want_lin=True)")
            lin = (_lin_combiner(lin_combiner), lin_bias)

        def res(out, fm, lo):
            return (out, fm, lo) if want_lin else (out, fm)
        self.stats["bag_lookups"] = self.stats.get("bag_lookups", 0) + 1
        check = self._collective()
        while True:
            cap_e, cap_b = self._bag_caps(B, values.numel())
            plan = self._bag_plan(B, cap_e, cap_b)
            self.stats["bag_cap"] = (cap_e, cap_b)
            host = self._bag_host() if check and values.device.type == "cuda" else None
            out, fm, pend, lo = self._bags_pipeline(plan, host, values, offsets, weights, B, combiner, max_norm, field_major, flags, want_fm,
                                                    lin)
            if not check:
                return res(out, fm, lo)
            if self.check != "eager":
                prev, self._bag_unchecked = self._bag_unchecked, (self._bag_unchecked + [pend])[-2:]
                if self.check == "lazy":          # the earlier lookups' verdicts: their header scans finished long ago
                    self._bag_unchecked = [pend]
                    if any([self._bag_verdict(p) for p in prev]):
                        raise RuntimeError("ShardedTables: a slab of the previous lookup_bags overflowed: that result was incomplete "
                                           "(the capacities have grown to %s)" % (self._bag_cap,))
                return res(out, fm, lo)
            if not self._bag_verdict(pend):       # the verdict, read after the whole lookup has been enqueued
                return res(out, fm, lo)

    def _bags_pipeline(self, plan, host, values, offsets, weights, B, combiner, max_norm, field_major, flags, want_fm, lin=None):
        """One pass of the bag lookup over `plan`'s buffers: bucket, exchange, pool on the owner, exchange, combine.  -> (emb, fm | None,
        pending verdict | None, lin | None).  With several ranks the pooling pass leaves [overflow, demands] off the received headers in
        plan.stat; the pending verdict is (event, host) after which the pinned `host` words hold them, or (None, a copy) on a CPU backend.
        What is done with it is the caller's policy.
        lin = (linear combiner, bias | None): the first-order term rides along -- the owner pools the first-order weights of each run
        right after the rows, one float per partial-row position goes back behind the partial rows (a second equal-split all-to-all), and
        the requester combines them beside the rows; without it nothing here changes."""
        F, K, be = self.F, self.K, self.backend
        cap_e, cap_b = plan.cap_e, plan.cap_b
        sb, sf = (1, B) if field_major else (F, 1)
        dev = values.device
        check = self._collective()
        be.bags_bucket(values, offsets, weights, B, sb, sf, combiner, flags, cap_e, cap_b, plan.send, plan.pos, plan.mask, plan.denom, plan.ws)
        _wait(self._a2a_equal(plan.recv, plan.send))
        be.bags_pool(plan.recv, cap_e, cap_b, max_norm, plan.rows, stat=plan.stat if check else None)
        pend = None
        if check and host is not None:
            host.copy_(plan.stat, non_blocking=True)
            pend = (torch.cuda.current_stream(dev).record_event(), host)
        elif check:
            pend = (None, plan.stat.clone())
        wr, wl = self._a2a_equal(plan.back, plan.rows), None
        if lin is not None:                      # (the owner's second pass runs under the row exchange where the transport is asynchronous)
            lrows, lback, lden = plan.lin_buffers()
            be.bags_linear_pool(plan.recv, cap_e, cap_b, lrows)
            wl = self._a2a_equal(lback, lrows)
        _wait(wr)
        out = torch.empty((B, F * K), dtype=torch.float32, device=dev)
        fm = torch.empty((B, 1), dtype=torch.float32, device=dev) if want_fm else None
        be.bags_combine(plan.back, cap_b, plan.pos, plan.mask, plan.denom, B, combiner, out, fm)
        lo = None
        if lin is not None:
            _wait(wl)
            lo = torch.empty((B, 1), dtype=torch.float32, device=dev)
            be.bags_linear_combine(lback, cap_b, plan.pos, plan.mask, values, offsets, weights, B, sb, sf, flags, lin[0], lden, lin[1], lo)
        return out, fm, pend, lo

    def _bag_args(self, values, offsets, weights, what):
        F = self.F
        if values.dim() != 1 or offsets.dim() != 1 or (offsets.numel() - 1) % F:
            raise ValueError("%s: values [nnz], offsets [B*F+1] with F=%d" % (what, F))
        if weights is not None and weights.numel() != values.numel():
            raise ValueError("%s: weights must be [nnz]" % what)
        return (offsets.numel() - 1) // F

    def lookup_bags_train(self, values, offsets, weights=None, combiner="mean", max_norm=None, field_major=False, flags=0,
                          with_linear=False, lin_combiner="sum"):
        """Differentiable lookup_bags (the same arguments but want_fm): emb [B_local, F*K] with a grad_fn, equal to lookup_bags(...)[0] bit
        for bit; the tables get no .grad.  emb.backward(g) performs ONE synchronous sparse Adagrad step over the global batch on every
        rank's shard (the optimiser of enable_training, shared with lookup_train): entry e of bag (b, f) contributes w_e * c_bag *
        g[b, f*K:(f+1)*K] to its row (c_bag = 1 / denom for mean and sqrtn, 1 for sum; through the slot's max_norm clip derivative at the
        row's pre-update value), and all contributions to a row -- inside a bag, across bags, across ranks -- are summed before its
        accumulator moves.  Entries the forward drops contribute nothing.
        The backward is the forward's exchange in reverse: the requester puts c_bag * g[b, f] where each partial row came back from, the
        same equal-split all-to-all carries at most min(L, P) gradient rows per bag back to the owners, and each owner runs the sorted
        Adagrad over the bag records it kept (include/dir_hip.h: dir_shard_bags_grad_f32, dir_sparse_adagrad_sorted_bags_f32).
        Training uses its own plans: inference lookups in between leave the backward's buffers alone.  The forward reads its own overflow
        verdict (every rank the same words) and repeats with grown capacities; verdicts pending from check="lazy" / "never" lookup_bags
        calls stay pending.  As with lookup_train, where duplicate contributions sit in the slabs depends on atomic order: once a row has
        duplicates, results agree to fp32 rounding, not bit for bit, from run to run.  Every rank must call it (SPMD).
        with_linear: -> (emb, lin) from ONE autograd node; lin [B_local, 1] = lookup_bags(want_lin=True, lin_combiner=)'s term without a
        bias (the bias is a replicated dense variable of the caller's).  Its backward receives both gradients: the requester scatters both
        (d lin[b] times 1 / the linear denominator for mean and sqrtn, to the position of every partial), the rows travel back, then the
        floats, and every owner applies Adagrad to its embedding rows, then FTRL (enable_linear_training) to its first-order rows over
        the same bag records on the Adagrad step's sort: entry e contributes w_e * c_bag * d lin[b], all contributions to a row summed
        before n, z and w move -- one optimiser step.
        Under enable_training_adam the owners take TF's sparse Adam step over the same records instead: the row's
        summed record gradient through the max_norm clip derivative is the gradient whose per-table norm is summed over the ranks and
        clipped, every local row moves, and two identical steps end bitwise equal (the run sums are formed in double).  Needs a backend
        with bags_adam_norm / bags_adam_apply; with_linear=True and graph capture are refused there, before anything is enqueued."""
        self._no_groups("lookup_bags_train")
        if self.optimizer is None:
            raise RuntimeError("call enable_training(lr) first")
        if self._adam:
            if not all(hasattr(self.backend, n) for n in ("bags_adam_norm", "bags_adam_apply")):
                raise NotImplementedError("lookup_bags_train under enable_training_adam: this backend has no owner-side Adam over bag records "
                                          "(bags_adam_norm / bags_adam_apply)")
            if with_linear:
                raise NotImplementedError("lookup_bags_train(with_linear=True) under enable_training_adam: the first-order rows' FTRL rides on "
                                          "the Adagrad step's sort")
            self._refuse_adam_capture(values)            # before anything is enqueued, not first inside backward()
        lin_comb = None
        if with_linear:
            self._need_linear("lookup_bags_train(with_linear=True)")
            self._units1("lookup_bags_train(with_linear=True)")
            if self._lin_hp is None:
                raise RuntimeError("call enable_linear_training(lr) first")
            lin_comb = _lin_combiner(lin_combiner)
        self._bag_args(values, offsets, weights, "lookup_bags_train")
        anchor = torch.zeros((), dtype=torch.float32, device=values.device, requires_grad=True)
        return _ShardedBagLookup.apply(self, values, offsets, weights, combiner, max_norm, field_major, flags, torch.is_grad_enabled(), lin_comb,
                                       anchor)

    def _bag_train_plan(self, B, cap_e, cap_b):
        key = (B, cap_e, cap_b)
        plan = self._bag_train_plans.get(key)
        if plan is not None and not plan.busy:
            return plan
        fresh = _BagPlan(self, B, cap_e, cap_b, train=True)
        if plan is None:                    # (a plan still held by a forward whose backward has not run is left to it)
            if len(self._bag_train_plans) >= 4:
                self._bag_train_plans = {k: v for k, v in self._bag_train_plans.items() if v.busy}
            self._bag_train_plans[key] = fresh
        return fresh

    def _bags_forward_train(self, values, offsets, weights, combiner, max_norm, field_major, flags, hold, lin_comb=None):
        B = self._bag_args(values, offsets, weights, "lookup_bags_train")
        self.stats["bag_train_lookups"] = self.stats.get("bag_train_lookups", 0) + 1
        while True:
            plan = self._bag_train_plan(B, *self._bag_caps(B, values.numel()))
            out, _, pend, lo = self._bags_pipeline(plan, plan.host, values, offsets, weights, B, combiner, max_norm, field_major, flags, False,
                                                   None if lin_comb is None else (lin_comb, None))
            # this lookup's own verdict only (the same words on every rank: all ranks repeat together); pending lazy verdicts stay pending
            if pend is None or not self._bag_verdict(pend):
                plan.busy = bool(hold)
                return out, plan, lo

    def _bags_backward_apply(self, saved, g, g_lin=None):
        """g_lin (with_linear): d loss / d lin [B_local, 1].  The forward's float buffers carry it back behind the gradient rows; the
        owner's FTRL runs after its Adagrad, over the same bag records, on that step's sort."""
        plan, B, combiner, max_norm, lin_comb = saved
        be = self.backend
        self._refuse_adam_capture(g)                     # before anything is enqueued (the plan stays held by its forward)
        self._updates += 1
        try:
            g2 = g if g.dim() == 2 and (B == 0 or g.stride(1) == 1) else g.contiguous()
            # the partial rows' buffers are the gradient's: rows = what this rank sends, back = what it receives (the same at world 1)
            be.bags_grad(g2, plan.cap_b, plan.pos, plan.mask, plan.denom, B, combiner, plan.rows)
            if g_lin is not None:
                lrows, lback, lden = plan.lin_buffers()
                be.bags_linear_grad(g_lin, plan.cap_b, plan.pos, plan.mask, lden, B, lin_comb, lrows)
            _wait(self._a2a_equal(plan.back, plan.rows))
            if g_lin is not None:
                _wait(self._a2a_equal(lback, lrows))
            if self._adam:
                # norm pass, norm sum over the ranks (every rank, also one that received nothing: a collective), apply on the norm pass's sort
                norms = None
                if self._adam_clip > 0:
                    norms = self._sum_norm_shares(be.bags_adam_norm(self.optimizer, plan.recv, plan.cap_e, plan.cap_b, plan.back, max_norm))
                be.bags_adam_apply(self.optimizer, plan.recv, plan.cap_e, plan.cap_b, plan.back, max_norm, norms)
            else:
                be.bags_adagrad(self.optimizer, plan.recv, plan.cap_e, plan.cap_b, plan.back, max_norm)
            if g_lin is not None:
                be.bags_ftrl(plan.recv, plan.cap_e, plan.cap_b, lback, *self._lin_hp, sorted_by=self.optimizer)
        finally:
            plan.busy = False

    def lookup(self, ids, want_fm=False, out=None, fm=None, want_lin=False, lin=None, lin_bias=None):
        """ids [B_local, F] int64 (global row ids; < 0 or >= vocab_f -> zeros) -> emb [B_local, F*K] fp32
        (and the FM second-order logit [B_local, 1] when want_fm).  out / fm: preallocated results (stable addresses).
        want_lin: the first-order term lin [B_local, 1] (+ lin_bias) comes last -- (emb, lin) or (emb, fm, lin); see lookup_async."""
        return self.lookup_async(ids, want_fm=want_fm, out=out, fm=fm, want_lin=want_lin, lin=lin, lin_bias=lin_bias).result()


_MASKED = []      # (hipStream_t, ExternalStream) pairs kept alive for the life of the process


def _masked_stream(device, n_cus, which):
    """A HIP stream whose kernels may only run on n_cus of the 256 compute units (hipExtStreamCreateWithCUMask), wrapped for torch.
    The lookup's kernels and RCCL's run there; the interaction kernels on the caller's stream keep the rest of the chip, so a lookup
    prefetched under a CIN or a tower costs it those CUs for as long as the lookup runs instead of fragmenting every CU's residency.
    The CUs are spread evenly over the mask (one per 256 / n_cus bits: every XCD and shader engine contributes)."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    total = torch.cuda.get_device_properties(device).multi_processor_count
    n = max(1, min(int(n_cus), total))
    step = max(1, total // n)
    words = (total + 31) // 32
    mask = (ctypes.c_uint32 * words)()
    for k in range(n):
        bit = (k * step + which * (step // 2)) % total      # the two side streams take interleaved CUs
        mask[bit // 32] |= 1 << (bit % 32)
    st = ctypes.c_void_p()
    with torch.cuda.device(device):
        rc = hip.hipExtStreamCreateWithCUMask(ctypes.byref(st), ctypes.c_uint32(words), mask)
    if rc != 0 or not st.value:
        raise RuntimeError("hipExtStreamCreateWithCUMask failed (%d)" % rc)
    ext = torch.cuda.ExternalStream(st.value, device=device)
    _MASKED.append((st, ext))
    return ext


class _ShardedLookup(torch.autograd.Function):
    """emb (or, with_lin, (emb, lin): the lookup and the first-order term from ONE node) = ShardedTables.lookup(ids) with a backward that
    routes the row gradients (and d lin along the same exchange) to their owners and lets each owner apply the sparse Adagrad update to its
    embedding rows, then FTRL to its first-order rows -- one optimiser step; no gradient tensor is returned for the tables."""

    @staticmethod
    def forward(ctx, st, ids, with_lin, anchor, dedup=False):
        emb, ctx.saved, lin = st._forward_train(ids, with_lin, dedup)
        ctx.st = st
        if st.G > 1:                                     # row groups: G embedding matrices (+ lin) from the one node
            return tuple(emb) + ((lin,) if with_lin else ())
        return (emb, lin) if with_lin else emb

    @staticmethod
    def backward(ctx, g, *more):
        st = ctx.st
        if st.G > 1:
            gs, g_lin = (g,) + more[:st.G - 1], (more[st.G - 1] if len(more) >= st.G else None)
            st._backward_apply(ctx.saved, gs, None if g_lin is None else g_lin.contiguous())
            return None, None, None, None, None
        g_lin = more[0] if more else None
        st._backward_apply(ctx.saved, g, None if g_lin is None else g_lin.contiguous())
        return None, None, None, None, None


class _ShardedBagLookup(torch.autograd.Function):
    """emb (or, lin_comb given, (emb, lin): the bags and the first-order term over them from ONE node) = ShardedTables.lookup_bags(...) with a
    backward that sends every bag's gradient (and d lin behind it) back along its partial rows and lets each owner apply the sparse Adagrad
    update to its shard, then FTRL to its first-order rows, from the bag records it kept -- one optimiser step; no gradient tensor is
    returned for the tables."""

    @staticmethod
    def forward(ctx, st, values, offsets, weights, combiner, max_norm, field_major, flags, hold, lin_comb, anchor):
        emb, plan, lin = st._bags_forward_train(values, offsets, weights, combiner, max_norm, field_major, flags, hold, lin_comb)
        ctx.st, ctx.saved = st, (plan, emb.shape[0], combiner, max_norm, lin_comb)
        return emb if lin_comb is None else (emb, lin)

    @staticmethod
    def backward(ctx, g, g_lin=None):
        ctx.st._bags_backward_apply(ctx.saved, g, None if g_lin is None else g_lin.contiguous())
        return (None,) * 11


# ---- the dense (replicated) side of multi-GPU training -----------------------------------------------------------------
def allreduce_grads(params, group=None, bucket_bytes=64 << 20, average=False):
    """Sum (or average) the .grad of replicated parameters over the ranks: the gradients are packed into flat buckets of about
    `bucket_bytes` (xGMI is point-to-point: few large all-reduces, not one per tensor), every bucket's all_reduce is issued
    before the first is waited for, then the results are copied back.  Parameters without a gradient are skipped on every rank
    alike (the caller guarantees the ranks agree on which parameters have gradients)."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        return
    host_staged = _host_staged(grads[0], group)
    buckets, cur, size = [], [], 0
    for g in grads:
        if g.is_sparse:
            raise ValueError("allreduce_grads: dense gradients only (sharded tables update at their owners)")
        cur.append(g)
        size += g.numel() * g.element_size()
        if size >= bucket_bytes:
            buckets.append(cur)
            cur, size = [], 0
    if cur:
        buckets.append(cur)
    flats, works = [], []
    for b in buckets:
        flat = torch.cat([g.reshape(-1) for g in b])
        if host_staged:
            flat = flat.cpu()
        flats.append(flat)
        works.append(dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group, async_op=True))
    scale = 1.0 / dist.get_world_size(group) if average else 1.0
    for b, flat, w in zip(buckets, flats, works):
        w.wait()
        off = 0
        for g in b:
            n = g.numel()
            g.copy_(flat[off:off + n].view_as(g).to(g.device) * scale if average else flat[off:off + n].view_as(g))
            off += n


@torch.no_grad()
def xdeepfm_predict(model, tables, ids, linear_logit=None):
    """Inference logits [B_local, 1] of an xdeepfm.XDeepFM over ROW-SHARDED embedding tables (BASELINE config 5: the config the reference's
    README.md:28 model shards; partitioner precedent deepFM.py:163-167).  With check='eager' the lookup runs WITHOUT its finish pass
    (lookup_rows): per micro-batch the CIN layers and the tower read the received rows through the inverse positions
    (XDeepFM.forward_rows) -- the rank-local passes of the lookup are bucket + owner gather only; otherwise lookup() + forward_embedded().
    Bit for bit the same logits either way wherever a micro-batch and the whole batch take the same dense kernels (those are chosen by row
    count: ops.dense_small_covers / dense_mid_covers / TOWER_MIN_ROWS).  `model`'s own embedding tables are not used; linear_logit [B_local, 1]: the first-order term
    computed by the caller (extra linear-only columns: their 4-byte rows live wherever the caller keeps them).  linear_logit = None and
    first-order rows on the shards (ShardedTables.attach_linear): the term comes from the tables, riding on the same lookup, with
    `model`'s linear_bias if it has one."""
    amax = tables.absmax()
    B = ids.shape[0]
    from_tables = linear_logit is None and tables.lin_rows is not None
    bias = getattr(model, "linear_bias", None) if from_tables else None
    bias = bias.data.reshape(-1)[:1] if bias is not None else None
    with _eval_mode(model):
        if tables.check == "eager":
            out = torch.empty((B, 1), dtype=torch.float32, device=ids.device)
            if from_tables:
                handle = tables.lookup_rows_async(ids, want_lin=True, lin_bias=bias)
                chunks, linear_logit = handle.result(), handle.lin
            else:
                chunks = tables.lookup_rows(ids)
            for s, e, rows, inv in chunks:
                if e > s:
                    out[s:e] = model.forward_rows(rows, inv, None if linear_logit is None else linear_logit[s:e], absmax=amax)
            return out
        if from_tables:
            emb, linear_logit = tables.lookup(ids, want_lin=True, lin_bias=bias)
            return model.forward_embedded(emb, linear_logit, range_ok=ops.f16_range_ok(amax))
        return model.forward_embedded(tables.lookup(ids), linear_logit, range_ok=ops.f16_range_ok(amax))


class ShardedDeepFMTrainer:
    """One synchronous multi-GPU training step of a DeepFM: the embedding tables are row-sharded over the ranks
    (ShardedTables: lookup = two all-to-alls, backward = the row exchange reversed + the owner's sparse Adagrad), the dense
    tower is replicated and its gradients are summed with bucketed all-reduces.  This is the reference's between-graph
    replicated training on parameter servers (partitioned embedding variables, deepFM.py:163-167; Adagrad on them, :61; the
    canned head's SUM loss reduction, :72 -- so gradients ADD over workers) restated for one process per GPU.
    `model` supplies the tower (dnn_logit_fn) and F, K; its own embedding_weights are not used.
    linear = dict(lr=, l1=, l2=): the reference's third term, linear_logits (deepFM.py:199-223), trained with linear_optimizer='Ftrl'
    (:58).  The first-order weights live on the shards (tables.attach_linear: co-located with the embedding rows, owner-side FTRL over the
    global batch); `model`.linear_bias is replicated and takes a dense FTRL step with its gradient summed over the ranks (FTRL is not
    linear in the gradient: the all-reduce comes first), so it must not be among dense_optimizer's parameters.  step() and predict() then
    compute fm + dnn + lin, and so do step_bags() and predict_bags() over multi-hot bags: the owners pool the first-order weights of
    each bag beside its embedding rows and `model`.linear_sparse_combiner is applied on the requester (lookup_bags(want_lin=True),
    lookup_bags_train(with_linear=True)); a backend without the bag forms of the term raises NotImplementedError there.
    linear = None: the FM + DNN model, as before.
    dedup = True: step() runs the de-duplicated training exchange (lookup_train(dedup=True): each distinct (slot, row) of a tile travels
    once, the entries' gradients -- and, with linear=, d lin on the same sort -- are summed per slab position on the requester); the
    default keeps one slab position per entry and its bits."""

    def __init__(self, model, tables, lr_sparse, dense_optimizer, group=None, initial_accumulator_value=0.1, linear=None, dedup=False):
        self.model, self.tables, self.group = model, tables, group
        self.dedup = bool(dedup)
        name = type(self).__name__
        refuse_shared_columns(name, getattr(model, "dnn_feature_columns", None))
        self.dense_params = [p for n, p in model.named_parameters()
                             if not (n.startswith("embedding_weights") or n.startswith("linear_weights"))]
        self.dense_optimizer = dense_optimizer
        tables.enable_training(lr_sparse, initial_accumulator_value)
        self.linear = None
        if linear is not None:
            if tables.lin_rows is None:
                raise ValueError("%s(linear=...): the tables have no first-order weights (ShardedTables.attach_linear)" % name)
            bias = model.linear_bias
            if any(p is bias for grp in dense_optimizer.param_groups for p in grp["params"]):
                raise ValueError("%s(linear=...): linear_bias takes the FTRL step here; leave it out of dense_optimizer" % name)
            hp = (float(linear["lr"]), float(linear.get("l1", 0.0)), float(linear.get("l2", 0.0)))
            tables.enable_linear_training(*hp)
            self.linear = hp
            # the bias's FTRL slots ([TF-upstream] FtrlOptimizer: accumulator 0.1, linear 0)
            self.bias_accum = torch.full_like(bias.data, float(linear.get("initial_accumulator_value", 0.1)))
            self.bias_linear = torch.zeros_like(bias.data)

    _BAG_LINEAR = ("bags_linear_pool", "bags_linear_combine", "bags_linear_grad", "bags_ftrl")

    def _bag_linear(self):
        """Whether the multi-hot forms carry the first-order term (linear=...); checked BEFORE anything is read off the model."""
        if self.linear is None:
            return False
        if not all(hasattr(self.tables.backend, n) for n in self._BAG_LINEAR):
            raise NotImplementedError("ShardedDeepFMTrainer(linear=...): this backend has no first-order term over multi-hot bags "
                                      "(bags_linear_pool / _combine / _grad, bags_ftrl); use step() / predict() or linear=None")
        return True

    def step(self, ids, labels):
        """ids [B_local, F] global row ids, labels [B_local, 1] -> this rank's summed loss (detached)."""
        from . import autograd as ag
        m = self.model
        self.dense_optimizer.zero_grad(set_to_none=True)
        if self.linear is not None:
            m.linear_bias.grad = None
            emb, lin = self.tables.lookup_train(ids, with_linear=True, dedup=self.dedup)       # both shards' rows update inside backward()
            logits = ag.fm_logit(emb, m.F, m.K) + m.dnn_logit_fn(emb) + (lin + m.linear_bias)      # ... + linear_logits, deepFM.py:339
        else:
            emb = self.tables.lookup_train(ids, dedup=self.dedup)             # tables update inside backward()
            logits = ag.fm_logit(emb, m.F, m.K) + m.dnn_logit_fn(emb)         # fm_logit_fn + dnn_logit_fn, deepFM.py:337-338
        loss = self._loss_backward_dense_step(logits, labels)
        if self.linear is not None:
            self._bias_ftrl_step()
        return loss

    def _bias_ftrl_step(self):
        """The replicated bias: FTRL with the GLOBAL gradient (allreduce_grads has summed it: linear_bias is among dense_params)."""
        b = self.model.linear_bias
        with torch.no_grad():
            self.tables.backend.ftrl_dense(b.data, self.bias_accum, self.bias_linear, b.grad.contiguous(), *self.linear)

    def _loss_backward_dense_step(self, logits, labels):
        """The tail of a step: the SUM loss, backward (every owner's shard takes its step inside), the dense gradients summed over the
        ranks, the dense step.  -> this rank's summed loss (detached)."""
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels, reduction="sum")
        loss.backward()
        allreduce_grads(self.dense_params, self.group)
        self.dense_optimizer.step()
        return loss.detach()

    def step_bags(self, values, offsets, labels, weights=None, field_major=False):
        """step() over multi-hot bags (a history column of the reference's DeepFM, deepFM.py:53,77,84): lookup_bags_train with every
        column's combiner and max_norm, the FM + DNN logits, the SUM loss, backward (every owner's shard takes its Adagrad step), the
        dense gradients summed over the ranks and the dense step.  values / offsets / weights as lookup_bags; labels [B_local, 1] ->
        this rank's summed loss (detached).  linear=...: + (lin + linear_bias) with the model's linear_sparse_combiner over the same bags
        (deepFM.py:89-95, 255-275); the owners' first-order rows take their FTRL step inside backward, the bias its dense one, as in step()."""
        from . import autograd as ag
        with_lin = self._bag_linear()
        m = self.model
        self.dense_optimizer.zero_grad(set_to_none=True)
        comb = [c.combiner for c in m.dnn_feature_columns]
        kw = dict(combiner=comb, max_norm=m._max_norm(), field_major=field_major)
        if not with_lin:
            emb = self.tables.lookup_bags_train(values, offsets, weights, **kw)
            return self._loss_backward_dense_step(ag.fm_logit(emb, m.F, m.K) + m.dnn_logit_fn(emb), labels)
        m.linear_bias.grad = None
        emb, lin = self.tables.lookup_bags_train(values, offsets, weights, with_linear=True, lin_combiner=m.linear_sparse_combiner, **kw)
        loss = self._loss_backward_dense_step(ag.fm_logit(emb, m.F, m.K) + m.dnn_logit_fn(emb) + (lin + m.linear_bias), labels)
        self._bias_ftrl_step()
        return loss

    @torch.no_grad()
    def predict(self, ids):
        """Inference logits [B_local, 1] of the same FM + DNN model over the row-sharded tables.  Where the one-launch tower kernel covers
        the model (dense.tower_infer's gather form: K = 16, F <= 26, ReLU tower with a units = 1 head) the lookup runs WITHOUT its finish
        pass (lookup_consume): per micro-batch the tower kernel reads the received rows through the inverse positions and folds the FM
        term -- the [B, F*K] concatenation is never written; otherwise lookup(want_fm=True) + dnn_logit_fn.  Bit for bit the same logits."""
        from .dense import tower_infer
        m = self.model
        with _eval_mode(m):
            B = ids.shape[0]
            out = torch.empty((B, 1), dtype=torch.float32, device=ids.device)
            amax = self.tables.absmax()
            state = {"fused": True}

            def consumer(s, e, rows, inv):
                lg = tower_infer(m.hidden, None, m.activation, bns=m.bns if len(m.bns) else None, head=m.logits_layer,
                                 gather=(rows_as_tables(rows, m.F, absmax=amax), inv, None, True)) if state["fused"] else None
                if lg is None:                                      # not covered (or too few rows): the finish pass's job, here
                    state["fused"] = False
                    emb, fm = ops.gather_fm(rows_as_tables(rows, m.F), inv)
                    lg = m.dnn_logit_fn(emb, adds=(fm,), range_ok=ops.f16_range_ok(amax))
                out[s:e] = lg
            bias = m.linear_bias.data.reshape(-1)[:1] if self.linear is not None else None
            if m.units == 1 and self.tables.check == "eager":
                if self.linear is not None:               # the first-order term rides on the same lookup; added to both routes' logits
                    _, lin = self.tables.lookup_async(ids, consumer=consumer, want_lin=True, lin_bias=bias).result()
                    return out + lin
                self.tables.lookup_consume(ids, consumer)
                return out
            if self.linear is not None:
                emb, fm, lin = self.tables.lookup(ids, want_fm=True, want_lin=True, lin_bias=bias)
                return m.dnn_logit_fn(emb, adds=(fm,), range_ok=ops.f16_range_ok(amax)) + lin
            emb, fm = self.tables.lookup(ids, want_fm=True)
            return m.dnn_logit_fn(emb, adds=(fm,), range_ok=ops.f16_range_ok(amax))      # the SHARDED tables' magnitude, not the model's own

    @torch.no_grad()
    def predict_bags(self, values, offsets, weights=None, field_major=False):
        """Inference logits [B_local, 1] of the same FM + DNN model over multi-hot bags of the row-sharded tables (a history column of the
        reference's DeepFM, deepFM.py:53,77,84): lookup_bags(want_fm=True) with every column's combiner and max_norm, then the tower with
        the FM term added -- what predict() does for one-hot ids.  linear=...: the first-order term (the model's linear_sparse_combiner,
        + linear_bias) rides on the same lookup and is added to the logits."""
        with_lin = self._bag_linear()
        m = self.model
        with _eval_mode(m):
            comb = [c.combiner for c in m.dnn_feature_columns]
            kw = dict(combiner=comb, max_norm=m._max_norm(), field_major=field_major, want_fm=True)
            if not with_lin:
                emb, fm = self.tables.lookup_bags(values, offsets, weights, **kw)
                return m.dnn_logit_fn(emb, adds=(fm,), range_ok=ops.f16_range_ok(self.tables.absmax()))
            emb, fm, lin = self.tables.lookup_bags(values, offsets, weights, want_lin=True, lin_combiner=m.linear_sparse_combiner,
                                                   lin_bias=m.linear_bias.data.reshape(-1)[:1], **kw)
            return m.dnn_logit_fn(emb, adds=(fm,), range_ok=ops.f16_range_ok(self.tables.absmax())) + lin


class ShardedXDeepFMTrainer(ShardedDeepFMTrainer):
    """One synchronous multi-GPU training step of an xdeepfm.XDeepFM over row-sharded tables (BASELINE config 5, "the config that shards":
    the reference's README.md:28 model under deepFM.py:163-167's partitioner): the embedding rows and, with linear=, the first-order
    weights over the same categorical columns live on the shards (tables_from_model); the CIN, the tower and linear_bias are replicated.
    step() is lookup_train -> XDeepFM.forward_embedded (the model's own training kernels, autograd.CinStack and mlp_head, unchanged) -> the
    SUM-reduced cross entropy -> backward, inside which every owner takes Adagrad on its embedding rows, then FTRL on its first-order
    rows -> the dense gradients summed over the ranks -> the dense step.  Gradients ADD over the ranks: two ranks equal one step over the
    concatenated batch.  `model`'s own embedding_weights and linear_weights are unused (tables_from_model slices them into the shards); the
    tower's fp16-range verdict comes from the sharded tables.
    dedup (the default: Criteo-like ids repeat): the de-duplicated training exchange, the first-order gradient summed per slab position
    on the row gradient's sort (lookup_train(with_linear=True, dedup=True)).
    linear = dict(lr=, l1=, l2=, initial_accumulator_value=) as in ShardedDeepFMTrainer: the replicated linear_bias takes the dense FTRL
    step on its all-reduced gradient and must not be in dense_optimizer.  linear = None: the CIN + DNN model.
    One-hot ids only: step_bags / predict_bags raise NotImplementedError (bags under dedup are out of scope)."""

    def __init__(self, model, tables, lr_sparse, dense_optimizer, group=None, initial_accumulator_value=0.1, linear=None, dedup=True):
        refuse_shared_columns("ShardedXDeepFMTrainer", getattr(model, "dnn_feature_columns", None))
        if tables.F != model.m or tables.K != model.D or tables.G != 1:
            raise ValueError("ShardedXDeepFMTrainer: the tables must hold F=%d slots of K=%d floats (tables_from_model), got F=%d K=%d groups=%d"
                             % (model.m, model.D, tables.F, tables.K, tables.G))
        super().__init__(model, tables, lr_sparse, dense_optimizer, group, initial_accumulator_value, linear, dedup)

    @classmethod
    def tables_from_model(cls, model, group=None, linear=True, **kw):
        """The ShardedTables of `model` (every rank holds the same replicated model): slot f = the f-th embedding column; linear: + the
        first-order weights, which must be over the embedding columns' categoricals (they share the id exchange).  kw: ShardedTables'
        options (partitions=, chunks=, mode=, ...)."""
        refuse_shared_columns("ShardedXDeepFMTrainer.tables_from_model", model.dnn_feature_columns)
        if linear and not model._same_categoricals():
            raise ValueError("ShardedXDeepFMTrainer.tables_from_model(linear=True): the linear columns are not the embedding columns' "
                             "categoricals; pass linear=False and compute the first-order term beside the shards")
        tables = ShardedTables.from_full([p.data for p in ops.plain_list(model.embedding_weights)], group=group, **kw)
        if linear:
            tables.attach_linear_from_full([p.data for p in ops.plain_list(model.linear_weights)])
        return tables

    def step(self, ids, labels):
        """ids [B_local, F] global row ids, labels [B_local, 1] -> this rank's summed loss (detached)."""
        m = self.model
        if not m.training:
            m.train()
        self.dense_optimizer.zero_grad(set_to_none=True)
        range_ok = ops.f16_range_ok(self.tables.absmax())       # the SHARDED tables' magnitude, not the model's own (unused) tables'
        with torch.enable_grad():
            if self.linear is not None:
                m.linear_bias.grad = None
                emb, lin = self.tables.lookup_train(ids, with_linear=True, dedup=self.dedup)
                logits = m.forward_embedded(emb, lin + m.linear_bias, range_ok=range_ok)
            else:
                logits = m.forward_embedded(self.tables.lookup_train(ids, dedup=self.dedup), None, range_ok=range_ok)
            loss = self._loss_backward_dense_step(logits, labels)
        if self.linear is not None:
            self._bias_ftrl_step()
        return loss

    def step_bags(self, *a, **kw):
        raise NotImplementedError("ShardedXDeepFMTrainer: one-hot ids only (step / predict)")

    predict_bags = step_bags

    @torch.no_grad()
    def predict(self, ids):
        """Inference logits [B_local, 1] over the row-sharded tables: xdeepfm_predict(model, tables, ids)."""
        return xdeepfm_predict(self.model, self.tables, ids)


def _esmm_parts(model):
    """(ctr tower, cvr tower, ctr linear model | None, cvr linear model | None) of an esmm.ESMM / esmm.ESMM_W_D whose columns the row-sharded
    trainer covers; ValueError naming the column otherwise.  Table f of the sharded tables is the f-th embedding column in the input
    layer's (name-sorted) order."""
    from ._input import categorical_of
    from .feature_column import EmbeddingColumn, HashedCategoricalColumn, IdentityCategoricalColumn
    subs = (model.ctr_model, model.cvr_model)
    wd = hasattr(subs[0], "dnn")                       # esmm._BaseModelWD: dnn tower + linear model
    towers = tuple(s.dnn if wd else s for s in subs)
    linears = tuple(s.linear if wd else None for s in subs)
    if any(t is None for t in towers):
        raise ValueError("ShardedESMMTrainer: both sub-models need a dnn tower (dnn_feature_columns)")
    il = towers[0].input_layer
    for t in towers:
        refuse_shared_columns("ShardedESMMTrainer", t.input_layer.columns)
    dim = None
    for c in il.columns:
        cat = categorical_of(c)
        if not isinstance(c, EmbeddingColumn) or not isinstance(cat, (IdentityCategoricalColumn, HashedCategoricalColumn)):
            raise ValueError("ShardedESMMTrainer: column %r: one-hot embedding columns over identity / hashed categorical columns only" % c.name)
        if getattr(c, "max_norm", None):
            raise ValueError("ShardedESMMTrainer: column %r: max_norm is not carried by the sharded one-hot lookup" % c.name)
        dim = c.dimension if dim is None else dim
        if c.dimension != dim:
            raise ValueError("ShardedESMMTrainer: column %r: dimension %d, the other columns have %d (one common dimension)" % (c.name, c.dimension, dim))
    for lm in linears:
        if lm is None:
            continue
        cats = [categorical_of(c) for c in il.emb_cols]
        for i, c in enumerate(lm.columns):
            if i >= len(cats) or categorical_of(c) is not cats[i]:
                raise ValueError("ShardedESMMTrainer: linear column %r (position %d): the linear columns must be the dnn columns' categorical "
                                 "columns in the input layer's order (%s)" % (getattr(c, "name", c), i, [getattr(x, "name", x) for x in cats]))
        if len(lm.columns) != len(cats):
            raise ValueError("ShardedESMMTrainer: %d linear columns for %d dnn columns (linear-only columns are not covered): missing %r"
                             % (len(lm.columns), len(cats), getattr(cats[len(lm.columns)], "name", cats[len(lm.columns)])))
    return towers + linears


class ShardedESMMTrainer:
    """One synchronous multi-GPU training step of an esmm.ESMM / esmm.ESMM_W_D over row-sharded tables: the reference shards the wide &
    deep ESMM's variables with the same partitioner as DeepFM's (ESMM_wide_deep.py:213-217, 258-261).  ctr_model and cvr_model look up
    the same (slot, row) pairs, so their two embedding rows of an id live side by side on its owner (ShardedTables(groups=2)) and ONE id
    exchange, owner gather, row exchange and finish pass -- and ONE owner-side sort and Adagrad step -- serve both; ESMM_W_D's two linear
    models are a 2-unit first-order term riding on the same exchange (attach_linear([rows, 2]), owner-side FTRL on the Adagrad step's
    sort).  The towers are replicated; their gradients are summed with bucketed all-reduces.
    The loss is _get_loss's (ESMM.py:150-175): each task's cross entropy MEAN-reduced with its weight column.  The two weight sums (the
    sample counts without weight columns) are all-reduced once per step and every rank back-propagates sum_local(w * ce) / W_global, so the
    gradients that ADD over the ranks -- at the owners and in allreduce_grads -- are the global-batch mean loss's.
    linear = dict(lr=, l1=, l2=) for ESMM_W_D: the two linear biases are replicated and take dense FTRL steps on their all-reduced
    gradients here, so they must not be among dense_optimizer's parameters.  `model`'s own embedding tables and linear weights are not
    used (tables_from_model copies them into the shards)."""

    def __init__(self, model, tables, lr_sparse, dense_optimizer, group=None, linear=None, initial_accumulator_value=0.1):
        self.model, self.tables, self.group = model, tables, group
        self.ctr, self.cvr, self.ctr_lin, self.cvr_lin = _esmm_parts(model)
        il = self.ctr.input_layer
        if tables.G != 2 or tables.F != len(il.emb_cols) or tables.K != il.emb_cols[0].dimension:
            raise ValueError("ShardedESMMTrainer: the tables must hold 2 row groups of F=%d slots of K=%d floats (tables_from_model), got G=%d F=%d K=%d"
                             % (len(il.emb_cols), il.emb_cols[0].dimension, tables.G, tables.F, tables.K))
        self.dense_params = [p for n, p in model.named_parameters() if not ("embedding_weights" in n or ".linear.weights" in n)]
        self.dense_optimizer = dense_optimizer
        tables.enable_training(lr_sparse, initial_accumulator_value)
        self.linear = None
        if linear is not None:
            if self.ctr_lin is None:
                raise ValueError("ShardedESMMTrainer(linear=...): the model has no linear models (esmm.ESMM_W_D with linear_feature_columns)")
            if tables.lin_rows is None or tables.U != 2:
                raise ValueError("ShardedESMMTrainer(linear=...): the tables need the 2-unit first-order rows (tables_from_model / attach_linear([rows, 2]))")
            self.biases = [self.ctr_lin.bias, self.cvr_lin.bias]
            if any(p is b for grp in dense_optimizer.param_groups for p in grp["params"] for b in self.biases):
                raise ValueError("ShardedESMMTrainer(linear=...): the linear biases take the FTRL step here; leave them out of dense_optimizer")
            hp = (float(linear["lr"]), float(linear.get("l1", 0.0)), float(linear.get("l2", 0.0)))
            tables.enable_linear_training(*hp)
            self.linear = hp
            # the biases' FTRL slots ([TF-upstream] FtrlOptimizer: accumulator 0.1, linear 0)
            self.bias_accum = [torch.full_like(b.data, float(linear.get("initial_accumulator_value", 0.1))) for b in self.biases]
            self.bias_linear = [torch.zeros_like(b.data) for b in self.biases]
        elif self.ctr_lin is not None:
            raise ValueError("ShardedESMMTrainer: the model has linear models: pass linear=dict(lr=, l1=, l2=)")

    @classmethod
    def tables_from_model(cls, model, group=None, linear_initial_accumulator_value=0.1, **kw):
        """The grouped ShardedTables of `model` (every rank holds the same replicated model): slot f = the f-th embedding column in the
        input layer's order, group 0 = ctr_model's table, group 1 = cvr_model's; for ESMM_W_D also the 2-unit first-order rows, unit 0 =
        ctr_model's linear weights, unit 1 = cvr_model's.  kw: ShardedTables' options (partitions=, chunks=, mode=, ...)."""
        ctr, cvr, ctr_lin, cvr_lin = _esmm_parts(model)
        per = [[p.data for p in ops.plain_list(t.input_layer.embedding_weights)] for t in (ctr, cvr)]
        tables = ShardedTables.from_full_groups(per, group=group, **kw)
        if ctr_lin is not None:
            full_w = [torch.stack([a.data.reshape(-1), b.data.reshape(-1)], dim=1) for a, b in zip(ctr_lin.weights, cvr_lin.weights)]
            tables.attach_linear_from_full(full_w, linear_initial_accumulator_value)
        return tables

    def _global_sums(self, sums):
        """The per-task weight sums over ALL ranks (one all-reduce of two numbers, no host read)."""
        if not dist.is_initialized() or dist.get_world_size(self.group) == 1:
            return sums
        t = sums.cpu() if _host_staged(sums, self.group) else sums.clone()
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t.to(sums.device)

    def step(self, ids, labels, ctr_weights=None, ctcvr_weights=None):
        """ids [B_local, F] global row ids (the input layer's column order); labels {'click_label', 'convert_label'} ([B_local, 1] each) or
        a [B_local, 2] tensor in that order; ctr_weights / ctcvr_weights [B_local, 1]: the two weight columns, or None (weight 1).
        -> this rank's (ctr_loss, ctcvr_loss) contributions to the global-batch mean losses (detached; they ADD over the ranks)."""
        from .esmm import ctcvr_logits_of
        from .train_spec import weighted_sigmoid_cross_entropy
        B = ids.shape[0]
        if isinstance(labels, dict):
            click, convert = labels["click_label"], labels["convert_label"]
        else:
            click, convert = labels[:, 0:1], labels[:, 1:2]
        self.dense_optimizer.zero_grad(set_to_none=True)
        if self.linear is not None:
            for b in self.biases:
                b.grad = None
            (emb_ctr, emb_cvr), lin = self.tables.lookup_train(ids, with_linear=True)      # every owner's rows update inside backward()
        else:
            emb_ctr, emb_cvr = self.tables.lookup_train(ids)
        ctr_logits, cvr_logits = self.ctr.tower(emb_ctr, True), self.cvr.tower(emb_cvr, True)
        if self.linear is not None:                                                        # dnn_logits + linear_logits, ESMM_wide_deep.py:265-270
            ctr_logits = ctr_logits + (lin[:, 0:1] + self.biases[0])
            cvr_logits = cvr_logits + (lin[:, 1:2] + self.biases[1])
        ctcvr_logits = ctcvr_logits_of(ctr_logits, cvr_logits)
        ctr_sum, _ = weighted_sigmoid_cross_entropy(ctr_logits, click.reshape(B, 1), ctr_weights, "sum")
        ctcvr_sum, _ = weighted_sigmoid_cross_entropy(ctcvr_logits, convert.reshape(B, 1), ctcvr_weights, "sum")
        dev = ctr_logits.device
        local = torch.stack([w.to(device=dev, dtype=torch.float32).sum() if w is not None else torch.tensor(float(B), device=dev)
                             for w in (ctr_weights, ctcvr_weights)])
        den = self._global_sums(local)
        parts = torch.where(den > 0, torch.stack([ctr_sum, ctcvr_sum]) / den.clamp_min(1e-30), torch.zeros_like(den))
        parts.sum().backward()
        allreduce_grads(self.dense_params, self.group)
        self.dense_optimizer.step()
        if self.linear is not None:                        # FTRL is not linear in the gradient: the all-reduce came first
            with torch.no_grad():
                for b, n, z in zip(self.biases, self.bias_accum, self.bias_linear):
                    self.tables.backend.ftrl_dense(b.data, n, z, b.grad.contiguous(), *self.linear)
        out = parts.detach()
        return out[0], out[1]

    @torch.no_grad()
    def predict(self, ids):
        """-> {'ctr_logits', 'cvr_logits', 'ctcvr_logits'} [B_local, 1] each: the grouped inference lookup (the first-order term and the
        two biases riding along for ESMM_W_D), the sub-models' own tower routing with the SHARDED tables' magnitude, ops.esmm_head."""
        from .esmm import ctcvr_logits_of
        with _eval_mode(self.model):
            ok = ops.f16_range_ok(self.tables.absmax())
            if self.linear is not None:
                bias = torch.cat([b.data.reshape(-1)[:1] for b in self.biases])
                (emb_ctr, emb_cvr), lin = self.tables.lookup(ids, want_lin=True, lin_bias=bias)
            else:
                emb_ctr, emb_cvr = self.tables.lookup(ids)
            ctr_logits, cvr_logits = self.ctr.tower(emb_ctr, ok), self.cvr.tower(emb_cvr, ok)
            if self.linear is not None:
                ctr_logits, cvr_logits = ctr_logits + lin[:, 0:1], cvr_logits + lin[:, 1:2]
            return {"ctr_logits": ctr_logits, "cvr_logits": cvr_logits, "ctcvr_logits": ctcvr_logits_of(ctr_logits, cvr_logits)}


def _dcn_columns(model):
    """(the embedding columns in the input layer's name-sorted order = the sharded tables' slots, their common width) of a
    dcn.DeepCrossNetwork the row-sharded trainer covers; ValueError naming the column otherwise."""
    from .feature_column import EmbeddingColumn
    il = model.input_layer
    refuse_shared_columns("ShardedDCNTrainer", il.columns)
    cols = [c for c in il.columns if isinstance(c, EmbeddingColumn)]
    if not cols:
        raise ValueError("ShardedDCNTrainer: the model has no embedding columns to shard")
    dim = cols[0].dimension
    for c in cols:                       # weighted categorical columns, per-column combiners and max_norm travel with the bag lookup
        if c.dimension != dim:
            raise ValueError("ShardedDCNTrainer: column %r: dimension %d, the other columns have %d (one common dimension)" % (c.name, c.dimension, dim))
    return cols, dim


class ShardedDCNTrainer:
    """One synchronous multi-GPU training step of a dcn.DeepCrossNetwork over row-sharded embedding tables: the reference's train_op
    (DeepCrossNetwork.py:264-290: tf.train.AdamOptimizer, every variable's gradient clipped on its own with tf.clip_by_norm(g, 100), a
    decayed learning rate) with the embedding variables partitioned over the ranks.  The tables take the owner-side sparse Adam
    (ShardedTables.enable_training_adam: the clip norm of a table is summed over its owners, every row of every shard moves every
    step); the cross and deep parts are replicated, their gradients are summed with bucketed all-reduces and the per-tensor clip runs
    on the SUMMED gradients, then the dense Adam steps.  Everything the one-GPU step knows -- the schedule, TF's epsilon placement, the
    one-global-step bias corrections, l2_reg on the deep kernels -- IS train_spec.TrainStep; the tables' optimiser gets its lr_t from
    the loop that serves TrainStep.sparse_adam.
    The loss is _create_loss's MEAN over the GLOBAL batch: every rank back-propagates its summed cross entropy / the all-reduced batch
    size, so the gradients that ADD over the ranks -- at the owners and in the all-reduce -- are the global mean loss's.  The l2_reg
    term is a function of replicated weights: every rank adds l2_reg / P of it, so its gradient counts once after the sum.
    Batch-norm statistics stay per rank: each rank normalises its own local batch and keeps its own moving averages, as each of the
    reference's workers does with the batch it reads.
    `model`'s embedding columns must share one width; its own embedding_weights are not used (tables_from_model copies them into the
    shards).  A batch with one id per sample and column takes the one-hot lookup (lookup_train; a column's max_norm is then the
    caller's to avoid: the one-hot lookup does not carry it and step() raises).  A batch with a multi-hot or weighted feature -- the
    reference's own input, safe_embedding_lookup_sparse (DeepCrossNetwork.py:126) -- takes lookup_bags_train with every column's
    combiner and max_norm, and the owners run the sparse Adam over the bag records; a backend without that form raises
    NotImplementedError at the first such batch.  weight_column and dnn_dropout raise NotImplementedError."""

    def __init__(self, model, tables, group=None):
        from .train_spec import CLIP_NORM, TrainStep
        self.model, self.tables, self.group = model, tables, group
        self.emb_cols, self.K = _dcn_columns(model)
        hp = model.hparams
        if hp.get("weight_column") is not None:
            raise NotImplementedError("ShardedDCNTrainer: weight_column (the weight sum would have to be all-reduced with the batch size)")
        if hp.get("dnn_dropout"):
            raise NotImplementedError("ShardedDCNTrainer: dnn_dropout")
        if tables.G != 1 or tables.F != len(self.emb_cols) or tables.K != self.K:
            raise ValueError("ShardedDCNTrainer: the tables must hold F=%d slots of K=%d floats (tables_from_model), got G=%d F=%d K=%d"
                             % (len(self.emb_cols), self.K, tables.G, tables.F, tables.K))
        P = dist.get_world_size(group) if dist.is_initialized() else 1
        self.dense_params = [p for n, p in model.named_parameters() if "embedding_weights" not in n]
        self.train = TrainStep(model, optimizer=hp.get("optimizer") or "Adam", optimizer_spec=hp.get("optimizer_spec"),
                               learning_rate_spec=hp.get("learning_rate_spec"), l2_reg=(hp["l2_reg"] / P if hp.get("l2_reg") else None),
                               l2_params=[lin.weight for lin in model.hidden], params=self.dense_params,
                               after_backward=lambda: allreduce_grads(self.dense_params, self.group))
        if self.train._tf_adam_eps is None:
            raise ValueError("ShardedDCNTrainer: the owner-side update is the reference's Adam (optimizer='Adam')")
        tables.enable_training_adam(self.train._beta1, self.train._beta2, self.train._tf_adam_eps, CLIP_NORM)
        self.train.sparse_adam.append(tables.optimizer)            # lr_t of the shards from the loop that serves the one-GPU tables

    @classmethod
    def tables_from_model(cls, model, group=None, **kw):
        """The ShardedTables of `model` (every rank holds the same replicated model): slot f = the f-th embedding column in the input
        layer's name-sorted order.  kw: ShardedTables' options (partitions=, chunks=, mode=, ...)."""
        cols, _ = _dcn_columns(model)
        il = model.input_layer
        full = ops.plain_list(il.embedding_weights)
        return ShardedTables.from_full([full[il.emb_cols.index(c)].data for c in cols], group=group, **kw)

    @property
    def global_step(self):
        return self.train.global_step

    def _x0(self, features, train):
        """The input layer's output over the sharded tables: the columns in name-sorted order, embedding columns as slices of the looked-up
        matrix (runs of adjacent ones as one slice), numeric and indicator columns as the input layer forms them.  (torch plumbing.)"""
        from ._input import collect_ids
        from .feature_column import EmbeddingColumn, NumericColumn
        il, dev, K = self.model.input_layer, self.tables.device, self.K
        got = collect_ids(self.emb_cols, features, dev)
        if got[0] == "onehot":
            if any(getattr(c, "max_norm", None) for c in self.emb_cols):
                raise ValueError("ShardedDCNTrainer: max_norm is not carried by the sharded one-hot lookup (feed the columns as bags)")
            ids = got[1]
            B = ids.shape[0]
            emb = self.tables.lookup_train(ids) if train else self.tables.lookup(ids)
        else:                            # ("ragged", values, offsets, weights, B): field-major bags, every column's own combiner and max_norm
            _, values, offsets, weights, B = got
            comb = [c.combiner for c in self.emb_cols]
            mn = [float(getattr(c, "max_norm", None) or 0.0) for c in self.emb_cols]
            mn = mn if any(mn) else None
            if train:
                emb = self.tables.lookup_bags_train(values, offsets, weights, combiner=comb, max_norm=mn, field_major=True)
            else:
                emb = self.tables.lookup_bags(values, offsets, weights, combiner=comb, max_norm=mn, field_major=True)[0]
        pieces, f, run0 = [], 0, None
        for c in list(il.columns) + [None]:
            if isinstance(c, EmbeddingColumn):
                run0 = f if run0 is None else run0
                f += 1
                continue
            if run0 is not None:
                pieces.append(emb[:, run0 * K:f * K])
                run0 = None
            if isinstance(c, NumericColumn):
                pieces.append(features[c.key].to(device=dev, dtype=torch.float32).reshape(-1, c.dimension))
            elif c is not None:
                pieces.append(il._indicator(c, features, dev, B))
        return (pieces[0] if len(pieces) == 1 else torch.cat(pieces, dim=1)), B

    def _global_batch(self, B, device):
        """The batch size over ALL ranks as a device scalar (one all-reduce of one number: on the host for gloo, no host read otherwise)."""
        t = torch.tensor([float(B)], dtype=torch.float32)
        if not dist.is_initialized() or dist.get_world_size(self.group) == 1:
            return t.to(device)
        if dist.get_backend(self.group) == "gloo":
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
            return t.to(device)
        t = t.to(device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    def step(self, features, labels):
        """features: the dict the model takes (this rank's local batch); labels [B_local, 1] -> this rank's share of the global-batch
        mean loss, its l2 share included (detached; the shares ADD over the ranks)."""
        from ._input import raise_pending
        x0, B = self._x0(features, True)                   # every owner's rows update inside backward()
        logits = self.model(x0)
        raise_pending()
        y = labels.to(device=logits.device, dtype=torch.float32).reshape(logits.shape)
        total = torch.nn.functional.binary_cross_entropy_with_logits(logits, y, reduction="sum")
        loss, _ = self.train(total / self._global_batch(B, logits.device).clamp_min(1.0).squeeze(0))
        return loss

    @torch.no_grad()
    def predict(self, features):
        """The model's predictions dict for this rank's local batch, x0 assembled from the inference lookup in the same way."""
        from ._input import raise_pending
        with _eval_mode(self.model):
            x0, _ = self._x0(features, False)
            out = self.model.predict(x0)
            raise_pending()
            return out


class ShardedDINTrainer:
    """One synchronous multi-GPU training step, and inference, of a din.DIN whose goods table (BASELINE config 4: 10 M x 64 plus its
    accumulator -- the table that outgrows one GPU first) is row-sharded over the ranks.  Every DIN kernel takes (table, history ids,
    lengths, candidate ids) and reads rows only through the ids, so the unit, its fused backward and the PReLU / Dice row-list path run
    UNCHANGED with table = the received rows of a sharded lookup and ids = the entries' positions in them: the [B, T + 1] entries (history,
    then the candidate) are flattened to a one-slot lookup without a finish pass, de-duplicated -- a sample's 51 entries repeat heavily
    across samples -- and in training the sparse gradient the model leaves on the received rows goes back through
    ShardedTables.lookup_rows_train's backward_rows (per-position sums on the requester, the reversed exchange, the owner's Adagrad).
    The dense parameters (the unit's MLP, the 200-80 tower) are replicated; their gradients are summed with bucketed all-reduces.
    Semantics: the loss is the SUM-reduced binary cross entropy, so gradients ADD over the ranks -- one step equals the single-process step
    over the concatenated batch.  Dice's batch statistics and moving averages are per rank, like an unsynchronised batch norm.
    `model`'s feature_columns are replicated dense-side parameters; a column whose parameter would get a sparse gradient (an embedding
    column) raises NotImplementedError.  `model`'s own attention.table is not used (tables_from_model copies it into the shards).
    dedup: the training exchange sends each distinct row of a tile once (lookup_rows_train(dedup=))."""

    def __init__(self, model, tables, lr_sparse, dense_optimizer, group=None, initial_accumulator_value=0.1, dedup=True):
        self.model, self.tables, self.group, self.dedup = model, tables, group, bool(dedup)
        il = model.input_layer
        if il is not None and len(il.embedding_weights):
            raise NotImplementedError("ShardedDINTrainer: feature_columns are replicated dense-side parameters; an embedding column's table "
                                      "gets a sparse gradient (use numeric / indicator columns, or shard the column's table)")
        if tables.G != 1 or tables.F != 1 or tables.K != model.K:
            raise ValueError("ShardedDINTrainer: the tables must hold the one goods table of K=%d floats (tables_from_model), got G=%d F=%d K=%d"
                             % (model.K, tables.G, tables.F, tables.K))
        if tables.check != "eager":
            raise ValueError("ShardedDINTrainer needs check='eager' (lookup_rows: an overflow is repaired before the rows are handed out)")
        self.dense_params = [p for n, p in model.named_parameters() if n != "attention.table"]
        self.dense_optimizer = dense_optimizer
        tables.enable_training(lr_sparse, initial_accumulator_value)

    @classmethod
    def tables_from_model(cls, model, group=None, **kw):
        """The one-table ShardedTables of `model`'s goods table (every rank holds the same replicated model).  kw: ShardedTables' options;
        inference lookups are de-duplicated unless dedup=False is given."""
        kw.setdefault("dedup", True)
        return ShardedTables.from_full([model.attention.table.data], group=group, **kw)

    def _entries(self, features):
        """[B, T + 1] int64 on the tables' device: the history ids -- positions at or beyond the sample's length set to -1, negative ids stay
        padding -- then the candidate id."""
        hk, lk, ck = self.model.keys
        dev = self.tables.device
        hist = features[hk].to(device=dev, dtype=torch.int64)
        cand = features[ck].to(device=dev, dtype=torch.int64).reshape(-1, 1)
        hist_len = features.get(lk) if hasattr(features, "get") else None
        if hist_len is not None:
            T = hist.shape[1]
            n = hist_len.to(device=dev, dtype=torch.int64).reshape(-1, 1).clamp(0, T)
            hist = torch.where(torch.arange(T, device=dev).unsqueeze(0) < n, hist, torch.full_like(hist, -1))
        return torch.cat([hist, cand], dim=1).contiguous()

    def _arith(self):
        """The unit's arithmetic from the SHARDED table's magnitude (a rank-invariant collective decision, ShardedTables.absmax) -- never from
        the received rows (a pass and a host wait per call) nor from the model's own unused table."""
        a = self.model.attention
        return ops.din_arith_name(self.tables.absmax(), (a.W1, a.W2, a.W3))

    def _rows_of(self, entries):
        """The inference lookup without its finish pass -> (rows [R, K], inv [B, T + 1]): ONE matrix for the whole local batch (the plan's
        micro-batches sit in one buffer; chunk c's positions are offset by c * P * cap), because Dice's statistics and the packed unit's
        partition are per call."""
        st = self.tables
        B, T1 = entries.shape
        flat = entries.reshape(-1, 1)
        h = st.lookup_rows_async(flat)
        chunks = h.result()
        plan = h.lk.plan
        base = None if plan is None else plan.back_all.untyped_storage().data_ptr()
        if plan is None or any(rows.untyped_storage().data_ptr() != base for _, _, rows, _ in chunks):
            # the exact path (from the start, or an overflow's repair): one entry for the whole batch, and pruned entries have a position
            # too -- a zero row; the unit must see them as padding
            (_, _, rows, inv), = chunks
            inv = torch.where((flat >= 0) & (flat < st.vocab_dev[0]), inv.reshape(-1, 1), torch.full_like(flat, -1))
            return rows, inv.reshape(B, T1)
        span, first = st.P * plan.cap, {s: c for c, (s, e) in enumerate(plan.bounds)}
        parts = []
        for s, e, _, inv in chunks:
            c = first[s]
            parts.append((torch.where(inv < 0, inv, inv + c * span) if c else inv).reshape(-1))
        inv = torch.cat(parts) if parts else torch.empty(0, dtype=torch.int64, device=flat.device)
        return plan.back_all, inv.reshape(B, T1)

    @torch.no_grad()
    def predict(self, features):
        """Inference logits [B_local, 1] for the features dict DIN.forward takes: the entries looked up with lookup_rows (de-duplicated, no
        finish pass), the model run with the received rows as its table -- the whole local batch in ONE call of the unit.  Bit for bit the
        single-GPU model holding the full table."""
        m = self.model
        entries = self._entries(features)
        T = entries.shape[1] - 1
        arith = self._arith()
        with _eval_mode(m):
            rows, inv = self._rows_of(entries)
            return m(features, table=rows, ids=(inv[:, :T], inv[:, T]), arith=arith)

    def step(self, features, labels):
        """features: the dict DIN.forward takes (this rank's local batch); labels [B_local, 1] -> this rank's summed loss (detached).
        lookup_rows_train, the model's training forward over the received rows (the sigmoid unit's fused node, the row-list path for PReLU /
        Dice), the SUM loss, backward; the sparse gradient of the received rows -- the unit's history and candidate rows plus the candidate
        embedding's -- goes to backward_rows as it is (no dense [R, K] coalesce), where every owner's shard takes its step; then the dense
        gradients are summed over the ranks and the dense optimiser steps."""
        m = self.model
        self.dense_optimizer.zero_grad(set_to_none=True)
        entries = self._entries(features)
        B, T = entries.shape[0], entries.shape[1] - 1
        arith = self._arith()
        h = self.tables.lookup_rows_train(entries.reshape(-1, 1), dedup=self.dedup)
        rows = h.rows.detach().requires_grad_(True)
        inv = h.inv.view(B, T + 1)
        logits = m(features, table=rows, ids=(inv[:, :T], inv[:, T]), arith=arith)
        y = labels.to(device=logits.device, dtype=torch.float32).reshape(logits.shape)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, y, reduction="sum")
        loss.backward()
        g = rows.grad
        if g is None:
            idx, vals = torch.empty(0, dtype=torch.int64, device=rows.device), torch.empty((0, rows.shape[1]), dtype=torch.float32, device=rows.device)
        elif g.is_sparse:
            idx, vals = g._indices()[0], g._values()              # uncoalesced: backward_rows sums the entries of a position
        else:
            idx, vals = torch.arange(rows.shape[0], device=rows.device), g
        h.backward_rows(idx, vals)
        allreduce_grads(self.dense_params, self.group)
        self.dense_optimizer.step()
        return loss.detach()
