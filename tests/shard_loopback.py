"""P ranks of dir_amd.shard in ONE process: every rank's backend (shard.HipBackend on a GPU, or a NumPy stand-in of tests/shard_standin*.py)
is driven in the order ShardedTables drives it (_enqueue with chunks = 1, _exchange_exact, _backward_apply, _bags_pipeline,
_bags_backward_apply), over buffers shaped like _Plan / _BagPlan, with every all_to_all replaced by recv[r][s] = send[s][r] on slab
views.  No process group, no second process: any owner count 1 <= P <= 64 costs one process.

Every buffer a backend writes carries a tail of guard words (at least one slab long) behind it, inside the same allocation; the driver
checks after every step that no tail moved, so an index error at the P * cap end of a buffer is a failed assertion here and not a write
into somebody else's memory.  Every pipeline returns the intermediate buffers of every rank, not only the result: the tests compare the
kernels with the stand-ins step by step, on identical inputs.

A plain helper module: tests/test_shard_loopback.py (CPU, stand-ins on both sides) proves the emulated exchange and the call order against
the full-table references; tests/test_gpu_shard_loopback.py puts HipBackend in."""
import types

import numpy as np
import torch

GUARD64 = 0x5A5A5A5A5A5A5A5A      # the tail pattern (as int64 / int32 words; a float tail holds the same bits)
GUARD32 = 0x5A5A5A5A
JUNK64 = 0x7171717171717171       # what a buffer body holds before a backend writes it ("torch.empty" made visible; finite as floats)
JUNK32 = 0x71717171


def _bits(t):
    """An integer view of a buffer, word for word."""
    return t if t.dtype in (torch.int64, torch.int32) else t.view(torch.int32)


class Guards:
    """Allocates buffers with guard tails and checks the tails."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.items = []

    def alloc(self, name, rank, shape, dtype, tail, fill=None):
        """A contiguous buffer of `shape` with `tail` guard words behind it.  fill: None = the junk pattern, else a value.
        rank: whose buffer it is (check(step, rank) looks at that rank's buffers only: a backend is handed no others)."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = int(np.prod(shape)) if shape else 1
        tail = max(64, int(tail))
        wide = dtype == torch.int64
        words = torch.full((n + tail,), JUNK64 if wide else JUNK32, dtype=torch.int64 if wide else torch.int32, device=self.device)
        words[n:] = GUARD64 if wide else GUARD32
        full = words if words.dtype == dtype else words.view(dtype)
        body = full[:n].view(shape)
        if fill is not None:
            body.fill_(fill)
        self.items.append((name, full, n, rank))
        return body

    def check(self, step, rank=None):
        bad = []
        for name, full, n, owner in self.items:
            if rank is not None and owner != rank:
                continue
            tail = _bits(full)[n:]
            if not bool((tail == (GUARD64 if full.dtype == torch.int64 else GUARD32)).all()):
                bad.append(name)
        assert not bad, "after %s: guard words behind %s were overwritten" % (step, bad)


def exchange_equal(send, P):
    """The equal-split all_to_all of P ranks' buffers (each P equal slabs): -> recv with recv[r] slab s = send[s] slab r, as fresh
    tensors of the senders' shape (the caller copies them into its guarded receive buffers)."""
    views = [s.reshape(P, -1) for s in send]
    return [torch.stack([views[s][r] for s in range(P)]).reshape(send[r].shape) for r in range(P)]


def exchange_var(send, counts, starts, P, width=1):
    """The exact path's variable-split all_to_all: rank s sends send[s][starts[s][r] : starts[s][r] + counts[s][r]] (rows of `width`
    elements) to rank r; -> per receiver the segments of senders 0..P-1 concatenated."""
    out = []
    for r in range(P):
        segs = [send[s].reshape(-1, width)[starts[s][r]:starts[s][r] + counts[s][r]] for s in range(P)]
        out.append(torch.cat(segs, dim=0).reshape(-1) if width == 1 else torch.cat(segs, dim=0))
    return out


def pack_linear(local_weights, device, init):
    """This rank's first-order weights as packed 16-byte rows [w | n | z | -] of one arena (ShardedTables.attach_linear's layout)."""
    n_rows = [int(w.numel()) for w in local_weights]
    arena = torch.zeros(sum(n_rows) * 4 + 4, dtype=torch.float32, device=device)
    off = (-(arena.data_ptr() // 4)) % 4
    rows = []
    for w, v in zip(local_weights, n_rows):
        blk = arena[off:off + v * 4].view(v, 4)
        blk[:, 0] = w.detach().reshape(-1).to(device=device, dtype=torch.float32)
        blk[:, 1] = float(init)
        rows.append(blk)
        off += v * 4
    return rows, arena


def hip_factory(local, vocab, parts, first, P, K, device, custom):
    from dir_amd.shard import HipBackend
    vocab_dev = torch.tensor(vocab, dtype=torch.int64, device=device)
    parts_dev = torch.tensor(parts, dtype=torch.int32, device=device) if custom else None
    first_dev = torch.tensor(first, dtype=torch.int32, device=device) if custom else None
    return HipBackend(local, vocab_dev, P, parts_dev, first_dev)


def standin_factory(local, vocab, parts, first, P, K, device, custom):
    from tests.shard_standin_bags_linear import BagsLinearBackend
    return BagsLinearBackend(local, vocab, parts, first, P, K)


class Loopback:
    """P ranks' shards of full tables (torch fp32 [vocab_f, K], any device) and one backend per rank.
    lin_full: the full first-order weights [vocab_f] per slot (packed beside the shards like ShardedTables.attach_linear does)."""

    def __init__(self, full, P, factory, device="cpu", partitions=None, lin_full=None, acc0=0.1):
        from dir_amd.shard import partition_layout
        self.P, self.device = int(P), torch.device(device)
        self.vocab = [int(t.shape[0]) for t in full]
        self.F, self.K = len(full), int(full[0].shape[1])
        self.slices, self.local, self.be, self.lin_rows = [], [], [], []
        self._arenas = []
        for r in range(self.P):
            parts, first, sl = partition_layout(self.vocab, self.K, self.P, r, partitions)
            local = [t[s:e].detach().clone().contiguous().to(self.device) for t, (s, e) in zip(full, sl)]
            be = factory(local, self.vocab, parts, first, self.P, self.K, self.device, partitions is not None)
            if lin_full is not None:
                rows, arena = pack_linear([w.reshape(-1)[s:e] for w, (s, e) in zip(lin_full, sl)], self.device, acc0)
                be.attach_linear(rows, arena)
                self.lin_rows.append(rows)
                self._arenas.append(arena)
            self.slices.append(sl)
            self.local.append(local)
            self.be.append(be)
        self.parts, self.first = parts, first
        self.opt = None

    # ---- helpers ----
    def _dev(self, t):
        return None if t is None else t.to(self.device)

    def enable_training(self, lr, acc0=0.1):
        self.opt = [be.make_optimizer(lr, acc0) for be in self.be]
        return self

    def assembled(self):
        """The shards put back together: [vocab_f, K] float64 numpy per table."""
        out = [np.zeros((v, self.K)) for v in self.vocab]
        for r in range(self.P):
            for f, (s, e) in enumerate(self.slices[r]):
                out[f][s:e] = self.local[r][f].detach().cpu().numpy()
        return out

    def assembled_linear(self):
        """-> (w, n, z): [vocab_f] float64 numpy per slot."""
        out = [[np.zeros(v) for v in self.vocab] for _ in range(3)]
        for r in range(self.P):
            for f, (s, e) in enumerate(self.slices[r]):
                rows = self.lin_rows[r][f].detach().cpu().numpy()
                for c in range(3):
                    out[c][f][s:e] = rows[:, c]
        return tuple(out)

    def _copy_in(self, dst, src, guards, step):
        for d, s in zip(dst, src):
            d.copy_(s)
        guards.check(step)

    # ---- the fixed-capacity one-hot lookup (ShardedTables._enqueue, chunks = 1, collective) ----
    def onehot_lookup(self, ids, cap, dedup=False, want_fm=True, want_lin=False, bias=None):
        """ids[r] [B_r, F] int64 per rank -> per rank a namespace of every buffer of the pipeline (send, recv, inv, counts, flags, cstat,
        rows, back, stat, lrows, lback, out, fm, lin) plus .guards."""
        P, F, K = self.P, self.F, self.K
        G = Guards(self.device)
        slab = P * (cap + 1)
        R = []
        for r in range(P):
            i = self._dev(ids[r])
            B = int(i.shape[0])
            s = types.SimpleNamespace(B=B, ids=i, cap=cap, dedup=dedup)
            s.send = G.alloc("send%d" % r, r, slab, torch.int64, cap + 1)
            s.recv = G.alloc("recv%d" % r, r, slab, torch.int64, cap + 1)
            s.inv = G.alloc("inv%d" % r, r, max(1, B * F), torch.int64, F)[:B * F]
            s.counts = G.alloc("counts%d" % r, r, P, torch.int64, 64, fill=0)
            s.flags = G.alloc("flags%d" % r, r, 1, torch.int32, 64, fill=0)
            s.cstat = G.alloc("cstat%d" % r, r, 2, torch.int64, 64, fill=0)
            s.stat = G.alloc("stat%d" % r, r, 2, torch.int64, 64, fill=0)
            s.ws = self.be[r].new_workspace(self.device)
            s.rows = G.alloc("rows%d" % r, r, (P * cap, K), torch.float32, cap * K)
            s.back = G.alloc("back%d" % r, r, (P * cap, K), torch.float32, cap * K)
            s.out = G.alloc("out%d" % r, r, (B, F * K), torch.float32, F * K) if B else torch.empty((0, F * K), dtype=torch.float32, device=self.device)
            s.fm = (G.alloc("fm%d" % r, r, (B, 1), torch.float32, 64) if B else torch.empty((0, 1), dtype=torch.float32, device=self.device)) if want_fm else None
            if want_lin:
                s.lrows = G.alloc("lrows%d" % r, r, P * cap, torch.float32, cap, fill=0.0)
                s.lback = G.alloc("lback%d" % r, r, P * cap, torch.float32, cap, fill=0.0)
                s.lin = G.alloc("lin%d" % r, r, (B, 1), torch.float32, 64) if B else torch.empty((0, 1), dtype=torch.float32, device=self.device)
            R.append(s)
        for r, s in enumerate(R):
            self.be[r].bucket_cap(s.ids, cap, s.send, s.inv, s.counts, s.flags, s.ws, stat=s.cstat, dedup=dedup)
            G.check("bucket_cap of rank %d" % r, r)
        self._copy_in([s.recv for s in R], exchange_equal([s.send for s in R], P), G, "the id exchange")
        for r, s in enumerate(R):
            self.be[r].gather_slabs(s.recv, cap, s.rows)
            G.check("gather_slabs of rank %d" % r, r)
        self._copy_in([s.back for s in R], exchange_equal([s.rows for s in R], P), G, "the row exchange")
        if want_lin:
            for r, s in enumerate(R):
                self.be[r].linear_gather(s.recv, cap, s.lrows)
                G.check("linear_gather of rank %d" % r, r)
            self._copy_in([s.lback for s in R], exchange_equal([s.lrows for s in R], P), G, "the linear exchange")
        for r, s in enumerate(R):
            self.be[r].slab_stat(s.recv, P, cap, s.stat)
            G.check("slab_stat of rank %d" % r, r)
        for r, s in enumerate(R):
            s.inv2d = self.be[r].inv2d(s.inv, s.B, F, dedup)
            if s.B and want_lin:
                self.be[r].linear_finish(s.lback, s.inv2d, self._dev(bias), s.lin)
            if s.B:
                self.be[r].finish_chunk(s.back, s.inv2d, want_fm, s.out, s.fm if want_fm else None)
            G.check("finish of rank %d" % r, r)
        for s in R:
            s.guards = G
        return R

    # ---- the exact, variable-size lookup (_exchange_exact + _lookup_exact) ----
    def exact_lookup(self, ids, want_fm=True, want_lin=False, bias=None):
        P, F, K = self.P, self.F, self.K
        G = Guards(self.device)
        R = []
        for r in range(P):
            i = self._dev(ids[r])
            s = types.SimpleNamespace(B=int(i.shape[0]), ids=i)
            flat = i.reshape(-1).contiguous()
            s.payload, s.inv, s.send_counts, s.starts = self.be[r].bucket(flat)
            R.append(s)
        sc = [[int(v) for v in s.send_counts.tolist()] for s in R]
        st = [[int(v) for v in s.starts.tolist()] for s in R]
        rc = [[sc[s_][r] for s_ in range(P)] for r in range(P)]
        rst = [[sum(rc[r][:s_]) for s_ in range(P)] for r in range(P)]
        for r, (s, got) in enumerate(zip(R, exchange_var([s.payload for s in R], sc, st, P))):
            s.sc, s.rc = sc[r], rc[r]
            s.recv = got.contiguous()
            s.rows = self.be[r].gather_packed(s.recv)
        for r, (s, got) in enumerate(zip(R, exchange_var([s.rows for s in R], rc, rst, P, width=K))):
            n = s.B * F
            s.back = G.alloc("back%d" % r, r, (n, K), torch.float32, K) if n else torch.empty((0, K), dtype=torch.float32, device=self.device)
            s.back.copy_(got.reshape(n, K))
        if want_lin:
            for r, s in enumerate(R):
                s.lw = G.alloc("lw%d" % r, r, max(1, s.recv.numel()), torch.float32, 64)[:s.recv.numel()]
                self.be[r].linear_gather(s.recv, None, s.lw)
                G.check("linear_gather (flat payload) of rank %d" % r, r)
            for r, (s, got) in enumerate(zip(R, exchange_var([s.lw for s in R], rc, rst, P))):
                s.lback = got.contiguous()
                s.lin = torch.empty((s.B, 1), dtype=torch.float32, device=self.device)
                self.be[r].linear_finish(s.lback, s.inv.view(s.B, F), self._dev(bias), s.lin)
        for r, s in enumerate(R):
            s.out, s.fm = self.be[r].finish(s.back, s.inv, s.B, F, want_fm)
            G.check("finish of rank %d" % r, r)
            s.guards = G
        return R

    # ---- one one-hot training step (_forward_train on the fixed path + _backward_apply) ----
    def onehot_train(self, ids, g_emb, cap, g_lin=None, ftrl=None):
        """ids[r], g_emb[r] [B_r, F*K], g_lin[r] [B_r, 1] | None, ftrl = (lr, l1, l2).  -> the forward's namespaces with the backward's
        buffers added (grecv, pay, lgrad_send, lgrad_recv)."""
        P, F, K = self.P, self.F, self.K
        with_lin = g_lin is not None
        R = self.onehot_lookup(ids, cap, dedup=False, want_fm=False, want_lin=with_lin, bias=None)
        G = R[0].guards
        gsend = []
        for r, s in enumerate(R):
            g2 = self._dev(g_emb[r]).contiguous()
            gs = torch.zeros((P * cap + 1, K), dtype=torch.float32, device=self.device)
            if s.B:
                idx = torch.where(s.inv < 0, torch.full_like(s.inv, P * cap), s.inv)
                gs.index_copy_(0, idx, g2.reshape(-1, K))
            gsend.append(gs[:P * cap].contiguous())
        for s, got in zip(R, exchange_equal(gsend, P)):
            s.grecv = got
        if with_lin:
            for r, s in enumerate(R):
                s.g_lin = self._dev(g_lin[r]).contiguous()
                self.be[r].linear_grad(s.g_lin, self.be[r].inv2d(s.inv, s.B, F, False), s.lrows)
                G.check("linear_grad of rank %d" % r, r)
                s.lgrad_send = s.lrows.clone()
            self._copy_in([s.lback for s in R], exchange_equal([s.lrows for s in R], P), G, "the linear gradient exchange")
        for r, s in enumerate(R):
            slabs = s.recv.view(P, cap + 1)
            hdr = slabs[:, 0] & 0xffffffff
            pos = torch.arange(cap, device=self.device)
            s.pay = torch.where(pos.unsqueeze(0) < hdr.unsqueeze(1), slabs[:, 1:], torch.full_like(slabs[:, 1:], -1)).reshape(-1)
            self.be[r].apply_adagrad(self.opt[r], s.pay, s.grecv)
            if with_lin:
                self.be[r].apply_ftrl(s.pay, s.lback.view(-1), ftrl[0], ftrl[1], ftrl[2], sorted_by=self.opt[r])
            G.check("the owner-side update of rank %d" % r, r)
        return R

    # ---- multi-hot bags (_bags_pipeline) ----
    def bags_lookup(self, csr, Bs, combiner, max_norm, field_major, flags, cap_e, cap_b, want_fm=True, lin=None):
        """csr[r] = (values, offsets, weights | None) torch tensors, Bs[r] the local batch.  lin = (linear combiner, bias | None) or None.
        -> per rank: send, recv, pos, mask, denom, rows, back, stat, lrows, lback, lden, out, fm, lin."""
        P, F, K = self.P, self.F, self.K
        G = Guards(self.device)
        words = P * (cap_e + 1) * 2
        R = []
        for r in range(P):
            v, o, w = (self._dev(t) for t in csr[r])
            B = int(Bs[r])
            nb = B * F
            s = types.SimpleNamespace(B=B, values=v, offsets=o, weights=w, cap_e=cap_e, cap_b=cap_b)
            s.send = G.alloc("send%d" % r, r, words, torch.int64, (cap_e + 1) * 2)
            s.recv = G.alloc("recv%d" % r, r, words, torch.int64, (cap_e + 1) * 2)
            s.pos = G.alloc("pos%d" % r, r, max(1, nb * P), torch.int32, P)
            s.mask = G.alloc("mask%d" % r, r, max(1, nb), torch.int64, 64)
            s.denom = G.alloc("denom%d" % r, r, max(1, nb), torch.float32, 64)
            s.rows = G.alloc("rows%d" % r, r, (P * cap_b, K), torch.float32, cap_b * K)
            s.back = G.alloc("back%d" % r, r, (P * cap_b, K), torch.float32, cap_b * K)
            s.stat = G.alloc("stat%d" % r, r, 3, torch.int64, 64, fill=0)
            s.ws = self.be[r].new_bags_workspace(self.device)
            s.out = G.alloc("out%d" % r, r, (B, F * K), torch.float32, F * K) if B else torch.empty((0, F * K), dtype=torch.float32, device=self.device)
            s.fm = (G.alloc("fm%d" % r, r, (B, 1), torch.float32, 64) if B else torch.empty((0, 1), dtype=torch.float32, device=self.device)) if want_fm else None
            if lin is not None:
                s.lrows = G.alloc("lrows%d" % r, r, P * cap_b, torch.float32, cap_b, fill=0.0)
                s.lback = G.alloc("lback%d" % r, r, P * cap_b, torch.float32, cap_b, fill=0.0)
                s.lden = G.alloc("lden%d" % r, r, max(1, nb), torch.float32, 64, fill=1.0)
                s.lin = G.alloc("lin%d" % r, r, (B, 1), torch.float32, 64) if B else torch.empty((0, 1), dtype=torch.float32, device=self.device)
            R.append(s)
        for r, s in enumerate(R):
            s.sb, s.sf = (1, s.B) if field_major else (F, 1)
            self.be[r].bags_bucket(s.values, s.offsets, s.weights, s.B, s.sb, s.sf, combiner, flags, cap_e, cap_b, s.send, s.pos, s.mask, s.denom, s.ws)
            G.check("bags_bucket of rank %d" % r, r)
        self._copy_in([s.recv for s in R], exchange_equal([s.send for s in R], P), G, "the slab exchange")
        for r, s in enumerate(R):
            self.be[r].bags_pool(s.recv, cap_e, cap_b, max_norm, s.rows, stat=s.stat)
            G.check("bags_pool of rank %d" % r, r)
        self._copy_in([s.back for s in R], exchange_equal([s.rows for s in R], P), G, "the partial-row exchange")
        if lin is not None:
            for r, s in enumerate(R):
                self.be[r].bags_linear_pool(s.recv, cap_e, cap_b, s.lrows)
                G.check("bags_linear_pool of rank %d" % r, r)
            self._copy_in([s.lback for s in R], exchange_equal([s.lrows for s in R], P), G, "the linear exchange")
        for r, s in enumerate(R):
            self.be[r].bags_combine(s.back, cap_b, s.pos, s.mask, s.denom, s.B, combiner, s.out, s.fm)
            G.check("bags_combine of rank %d" % r, r)
            if lin is not None:
                self.be[r].bags_linear_combine(s.lback, cap_b, s.pos, s.mask, s.values, s.offsets, s.weights, s.B, s.sb, s.sf, flags, lin[0],
                                               s.lden, self._dev(lin[1]), s.lin)
                G.check("bags_linear_combine of rank %d" % r, r)
            s.guards = G
        return R

    # ---- one bag training step (_bags_forward_train + _bags_backward_apply) ----
    def bags_train(self, csr, Bs, g_emb, combiner, max_norm, field_major, flags, cap_e, cap_b, g_lin=None, lin_comb=None, ftrl=None):
        P = self.P
        with_lin = g_lin is not None
        R = self.bags_lookup(csr, Bs, combiner, max_norm, field_major, flags, cap_e, cap_b, want_fm=False,
                             lin=(lin_comb, None) if with_lin else None)
        G = R[0].guards
        for r, s in enumerate(R):
            s.pooled = s.rows.clone()                        # the forward's partial rows: the backward reuses the buffer
            s.g = self._dev(g_emb[r]).contiguous()
            self.be[r].bags_grad(s.g, cap_b, s.pos, s.mask, s.denom, s.B, combiner, s.rows)
            G.check("bags_grad of rank %d" % r, r)
            if with_lin:
                s.lpooled = s.lrows.clone()
                s.g_lin = self._dev(g_lin[r]).contiguous()
                self.be[r].bags_linear_grad(s.g_lin, cap_b, s.pos, s.mask, s.lden, s.B, lin_comb, s.lrows)
                G.check("bags_linear_grad of rank %d" % r, r)
        self._copy_in([s.back for s in R], exchange_equal([s.rows for s in R], P), G, "the gradient-row exchange")
        if with_lin:
            self._copy_in([s.lback for s in R], exchange_equal([s.lrows for s in R], P), G, "the linear gradient exchange")
        for r, s in enumerate(R):
            self.be[r].bags_adagrad(self.opt[r], s.recv, cap_e, cap_b, s.back, max_norm)
            if with_lin:
                self.be[r].bags_ftrl(s.recv, cap_e, cap_b, s.lback, ftrl[0], ftrl[1], ftrl[2], sorted_by=self.opt[r])
            G.check("the owner-side update of rank %d" % r, r)
        return R
