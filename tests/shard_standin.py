"""What the multi-process CPU tests of dir_amd.shard (tests/test_shard*_gloo.py) share: the NumPy stand-in for the HIP steps and the
harness that runs one function on every rank of a gloo group.

The exchange logic under test is exactly what runs on a GPU box under RCCL.  The HIP kernels cannot run without a GPU, so NumpyBackend
takes shard.HipBackend's place through ShardedTables' `backend` injection point, reading and writing the same buffers in the same
formats (include/dir_hip.h: the one-hot slabs with their packed headers, the bag slabs of 16-byte records, the packed first-order rows).
A change to a slab format or to a backend method's signature is made here once."""
import datetime
import os
import sys
import tempfile
import traceback

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CODES = {"sum": 0, "mean": 1, "sqrtn": 2}


def per_slot(x, F):
    return list(x) if isinstance(x, (list, tuple)) else [x] * F


# ---- the ranks ---------------------------------------------------------------------------------------------------------------------
def store():
    """A rendezvous token for one process group: the path of a FileStore file (no TCP port to clash on -- a port probed free here can be
    taken again before rank 0 binds it on a shared host)."""
    return os.path.join(tempfile.mkdtemp(prefix="dir_pg_"), "store")


def _rank_main(rank, world, path, body, args, q):
    try:
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        torch.set_num_threads(1)
        dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
        try:
            q.put((rank, body(rank, world, *args)))   # an assertion that fails on one rank ends that rank's run: its peers time out and say so
        finally:
            dist.destroy_process_group()
    except Exception:                                  # surface the reason instead of leaving the parent to time out
        q.put((rank, traceback.format_exc()))


def run_ranks(world, body, *args, timeout=300):
    """body(rank, world, *args) on every rank of a fresh gloo group, one spawned process per rank.  -> {rank: what body returned}; a rank
    that raised, or a process that did not exit cleanly, fails the calling test."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    path = store()
    procs = [ctx.Process(target=_rank_main, args=(r, world, path, body, args, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=timeout) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r for r, _ in res) == list(range(world))
    for rank, got in res:
        assert not isinstance(got, str), "rank %d raised:\n%s" % (rank, got)
    return dict(res)


def run_checked(world, scenarios, spec):
    """run_ranks for scenarios(rank, world, spec) -> ([(name, ok, detail), ...], ...): every named check must hold on every rank."""
    out = run_ranks(world, scenarios, spec)
    for rank, got in out.items():
        bad = [(n, d) for n, ok, d in got[0] if not ok]
        assert not bad, "rank %d: %s" % (rank, bad)
    return out


# ---- NumPy stand-ins for the HIP steps ---------------------------------------------------------------------------------------------
class NumpyBackend:
    """Every backend method the gloo tests need: both paths of the one-hot lookup (de-duplication, FM), its owner-side Adagrad (float64
    accumulators), the four steps of the linear term and ftrl_dense, the three bag steps and the bags' two training steps.  fp32
    arithmetic in the kernels' order where a test compares bit for bit (entries in entry order inside a partial, partials in ascending
    owner order, the linear sum in slot order)."""

    def __init__(self, local, vocab, parts, first, P, K):
        self.local, self.vocab, self.parts, self.first, self.P, self.K, self.F = local, vocab, parts, first, P, K, len(vocab)
        self.lin, self.U = None, 1
        self.ftrl_calls, self.ftrl_widths = 0, []

    def owner(self, f, ids):
        """owner rank, local row of ids (all inside [0, vocab_f)) of slot f."""
        from oracle import np_ref as R
        o, l = R.shard_div_owner(ids, self.vocab[f], self.parts[f])
        return (np.asarray(o) + self.first[f]) % self.P, np.asarray(l)

    def route(self, a):
        """owner rank / local row of every entry of a flat [.., F] id array (-1: pruned or out of range)."""
        F, n = self.F, a.size
        own, loc = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
        for f in range(F):
            sel = np.arange(f, n, F)
            ok = (a[sel] >= 0) & (a[sel] < self.vocab[f])
            o, l = self.owner(f, np.where(ok, a[sel], 0))
            own[sel] = np.where(ok, o, -1)
            loc[sel] = np.where(ok, l, -1)
        return own, loc

    # ---- exact path ----
    def bucket(self, flat):
        a = flat.numpy()
        n, F, P = a.size, self.F, self.P
        own, loc = self.route(a)
        own = np.where(own < 0, np.arange(n) % P, own)          # pruned entries travel as -1 payloads
        order = np.argsort(own, kind="stable")
        inv = np.empty(n, np.int64)
        inv[order] = np.arange(n)
        packed = np.where(loc < 0, -1, loc * F + (np.arange(n) % F))[order]
        counts = np.bincount(own, minlength=P).astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        return torch.from_numpy(packed), torch.from_numpy(inv), torch.from_numpy(counts), torch.from_numpy(starts)

    def gather_packed(self, payload):
        p = payload.numpy()
        out = np.zeros((p.size, self.K), np.float32)
        for i, v in enumerate(p):
            if v >= 0:
                out[i] = self.local[v % self.F].numpy()[v // self.F]
        return torch.from_numpy(out)

    def back_buffer(self, n, K, device):
        return torch.empty((n, K), dtype=torch.float32)

    def finish(self, back, inv, B, F, want_fm, out=None, fm=None):
        iv = inv.numpy()
        emb = np.where((iv >= 0)[:, None], back.numpy()[np.maximum(iv, 0)], 0).astype(np.float32).reshape(B, F * self.K)
        fmv = None
        if want_fm:
            from oracle import oracle as O
            fmv = torch.from_numpy(O.fm_second_order(emb, F, self.K).reshape(B, 1))
            if fm is not None:
                fm.copy_(fmv)
                fmv = fm
        emb = torch.from_numpy(emb)
        if out is not None:
            out.copy_(emb)
            emb = out
        return emb, fmv

    # ---- fixed-capacity path ----
    def new_workspace(self, device):
        return torch.zeros(64, dtype=torch.int32)

    def bucket_cap(self, ids2d, cap, payload, inv, counts, overflow, workspace, stat=None, dedup=False):
        a = ids2d.numpy().reshape(-1)
        F, P = self.F, self.P
        own, loc = self.route(a)
        pay = payload.numpy().reshape(P, cap + 1)
        iv = inv.numpy()
        iv[:] = -1
        fill = np.zeros(P, np.int64)
        seen = {}
        for i in range(a.size):
            o = own[i]
            if o < 0:
                continue
            p = loc[i] * F + (i % F)
            if dedup and (o, p) in seen:                 # an EXACT unique per owner (the HIP kernel's is per tile: same result)
                iv[i] = seen[(o, p)]
                continue
            if fill[o] < cap:
                pay[o, 1 + fill[o]] = p
                iv[i] = o * cap + fill[o]
            if dedup:
                seen[(o, p)] = iv[i]
            fill[o] += 1
        pay[:, 0] = np.minimum(fill, cap) | (int(fill.max()) << 32)   # header: valid slots | this sender's largest demand
        counts.copy_(torch.from_numpy(fill))
        overflow.fill_(int((fill > cap).any()))
        if stat is not None:
            stat[0], stat[1] = int((fill > cap).any()), int(fill.max())

    @staticmethod
    def inv2d(inv, Bc, F, dedup):
        return inv.view(Bc, F)

    def slab_stat(self, recv_all, n_slabs, cap, stat):
        h = recv_all.numpy().reshape(n_slabs, cap + 1)[:, 0] >> 32
        stat[0], stat[1] = int(h.max() > cap), int(h.max())

    def gather_slabs(self, recv, cap, out):
        r, o = recv.numpy().reshape(self.P, cap + 1), out.numpy()
        for s in range(self.P):
            for j in range(int(r[s, 0] & 0xffffffff)):
                v = r[s, 1 + j]
                o[s * cap + j] = self.local[v % self.F].numpy()[v // self.F]

    def finish_chunk(self, back, inv2d, want_fm, out, fm):
        b, f = inv2d.shape
        self.finish(back, inv2d.reshape(-1), b, f, want_fm, out=out, fm=fm)

    # ---- the owner-side Adagrad, shared by the one-hot and the bag steps ----
    def make_optimizer(self, lr, init):
        return {"lr": lr, "acc": [np.full(tuple(t.shape), init, np.float64) for t in self.local]}

    def _adagrad(self, opt, f, rows, g):
        """One Adagrad step of table f: rows (unique) take their summed gradient rows g (float64)."""
        w = self.local[f].numpy().astype(np.float64)
        acc = opt["acc"][f]
        acc[rows] += g * g
        w[rows] -= opt["lr"] * g / np.sqrt(acc[rows])
        self.local[f].copy_(torch.from_numpy(w.astype(np.float32)))

    def apply_adagrad(self, opt, payload, grad_rows):
        p, g = payload.numpy(), grad_rows.numpy().astype(np.float64)
        for f in range(self.F):
            sel = (p >= 0) & (p % self.F == f)
            gsum = np.zeros(tuple(self.local[f].shape))
            np.add.at(gsum, p[sel] // self.F, g[sel])              # ALL duplicates of a row are summed before its accumulator moves
            rows = np.unique(p[sel] // self.F)
            self._adagrad(opt, f, rows, gsum[rows])

    # ---- the linear term ----
    def attach_linear(self, rows, arena):
        # [local rows, 4 U] float32 torch tensors, U blocks [w | n | z | -] (one per unit) side by side: the kernels' buffers
        self.lin, self.U = rows, rows[0].shape[1] // 4

    def _weights_of(self, p):
        """U weights per payload word (0.0 for p < 0 and for rows outside the slot's local rows)."""
        out = np.zeros((p.size, self.U), np.float32)
        for i, v in enumerate(p):
            if v >= 0 and v // self.F < self.lin[v % self.F].shape[0]:
                out[i] = self.lin[v % self.F].numpy()[v // self.F, 0::4]
        return out

    def linear_gather(self, recv, cap, out):
        U, o = self.U, out.numpy()
        if cap is None:
            o[:recv.numel() * U] = self._weights_of(recv.numpy()).reshape(-1)
            return
        r = recv.numpy().reshape(self.P, cap + 1)
        o[:self.P * cap * U] = 0.0                     # every word is written: nothing uninitialised crosses the wire
        for s in range(self.P):
            nv = int(r[s, 0] & 0xffffffff)
            o[s * cap * U:(s * cap + nv) * U] = self._weights_of(r[s, 1:1 + nv]).reshape(-1)

    def linear_finish(self, wback, inv2d, bias, out):
        U = self.U
        iv, wb = inv2d.numpy(), wback.numpy().reshape(-1, U)
        acc = np.zeros((iv.shape[0], U), np.float32)
        for f in range(iv.shape[1]):                   # float32, slot order, per unit: dir_linear_onehot_rows_f32's sum
            acc = acc + np.where((iv[:, f] >= 0)[:, None], wb[np.maximum(iv[:, f], 0)], np.float32(0)).astype(np.float32)
        acc = acc + (bias.numpy().reshape(1, U).astype(np.float32) if bias is not None else np.float32(0))
        out.copy_(torch.from_numpy(acc.astype(np.float32)))

    def linear_grad(self, g, inv2d, send):
        U = self.U
        iv, gg, sd = inv2d.numpy(), g.detach().numpy().reshape(-1, U), send.numpy().reshape(-1, U)
        sd[:] = 0.0
        for b in range(iv.shape[0]):
            for f in range(iv.shape[1]):
                if iv[b, f] >= 0:
                    sd[iv[b, f]] = gg[b]

    @staticmethod
    def _ftrl(w, n, z, g, lr, l1, l2):
        """FTRL-Proximal in float64: -> (w, n, z) after the step with gradient g."""
        n_new = n + g * g
        z_new = z + g - (np.sqrt(n_new) - np.sqrt(n)) / lr * w
        return np.where(np.abs(z_new) > l1, (np.sign(z_new) * l1 - z_new) / (np.sqrt(n_new) / lr + 2 * l2), 0.0), n_new, z_new

    def apply_ftrl(self, payload, grad, lr, l1, l2, sorted_by=None):
        self.ftrl_calls += 1
        U = self.U
        p = payload.numpy()
        self.ftrl_widths.append(grad.numel() // max(1, p.size))      # floats per payload word, as the caller sent them
        g = grad.numpy().astype(np.float64).reshape(-1, U)
        assert g.shape[0] == p.size
        for f in range(self.F):
            sel = (p >= 0) & (p % self.F == f)
            rows = p[sel] // self.F
            r = self.lin[f].numpy()
            gs = np.zeros((r.shape[0], U))
            np.add.at(gs, rows, g[sel])                # ALL duplicates of a row are summed before n, z and w move
            t = np.zeros(r.shape[0], bool)
            t[rows] = True
            for u in range(U):
                c = 4 * u
                r[t, c], r[t, c + 1], r[t, c + 2] = self._ftrl(*(r[t, c + k].astype(np.float64) for k in range(3)), gs[t, u], lr, l1, l2)

    def ftrl_dense(self, w, accum, linear, grad, lr, l1, l2):
        new = self._ftrl(*(t.numpy().astype(np.float64) for t in (w, accum, linear, grad)), lr, l1, l2)
        for t, v in zip((w, accum, linear), new):
            t.copy_(torch.from_numpy(v.astype(np.float32)))

    # ---- multi-hot bags, pooled on the owner ----
    def _codes(self, combiner):
        return [_CODES[c] for c in per_slot(combiner, self.F)]

    def new_bags_workspace(self, device):
        return torch.zeros(256, dtype=torch.int32)

    def bags_bucket(self, values, offsets, weights, B, sb, sf, combiner, flags, cap_e, cap_b, slabs, pos, mask, denom, workspace):
        F, P = self.F, self.P
        vals, offs = values.numpy(), offsets.numpy()
        wts = None if weights is None else weights.numpy()
        prune = wts is not None and bool(flags & 1)
        cb_ = self._codes(combiner)
        sl = slabs.numpy().reshape(P, cap_e + 1, 2)
        ps, mk, dn = pos.numpy(), mask.numpy(), denom.numpy()
        ne, nb = np.zeros(P, np.int64), np.zeros(P, np.int64)
        for b in range(B):
            for f in range(F):
                g = b * F + f
                s0, s1 = offs[b * sb + f * sf], offs[b * sb + f * sf + 1]
                runs = {}
                wsum, w2sum, n = np.float32(0), np.float32(0), 0
                for e in range(s0, s1):
                    i = vals[e]
                    w = np.float32(1) if wts is None else np.float32(wts[e])
                    if i < 0 or i >= self.vocab[f] or (prune and not w > 0):
                        continue
                    o, l = self.owner(f, [i])
                    runs.setdefault(int(o[0]), []).append((int(l[0]) * F + f, w))
                    wsum = np.float32(wsum + w)
                    w2sum = np.float32(w2sum + np.float32(w * w))
                    n += 1
                if cb_[f] == 1:
                    dn[g] = wsum if wts is not None else np.float32(n)
                elif cb_[f] == 2:
                    dn[g] = np.sqrt(w2sum) if wts is not None else np.sqrt(np.float32(n))
                else:
                    dn[g] = 1.0
                m = 0
                for o in sorted(runs):
                    m |= 1 << o
                    q = nb[o]
                    nb[o] += 1
                    ps[g * P + o] = o * cap_b + q if q < cap_b else -1
                    for packed, w in runs[o]:
                        if ne[o] < cap_e:
                            ret = q if q < cap_b else -1
                            sl[o, 1 + ne[o], 0] = packed
                            sl[o, 1 + ne[o], 1] = int(np.float32(w).view(np.uint32)) | (int(np.uint32(ret & 0xffffffff)) << 32)
                        ne[o] += 1
                mk[g] = np.int64(np.uint64(m).astype(np.int64)) if m < (1 << 63) else np.int64(m - (1 << 64))
        de, db = int(ne.max()), int(nb.max())
        for o in range(P):
            sl[o, 0, 0] = min(ne[o], cap_e) | (min(nb[o], cap_b) << 32)
            sl[o, 0, 1] = de | (db << 32)

    def bags_pool(self, recv, cap_e, cap_b, max_norm, rows, stat=None):
        F, P = self.F, self.P
        sl = recv.numpy().reshape(P, cap_e + 1, 2)
        mn = per_slot(max_norm, F)
        out = rows.numpy()
        for s in range(P):
            ne = int(sl[s, 0, 0] & 0xffffffff)
            prev, acc = None, None
            for j in range(ne + 1):
                ret = int(np.int64(sl[s, 1 + j, 1]) >> 32) if j < ne else None
                if ret != prev and prev is not None and prev >= 0:
                    out[s * cap_b + prev] = acc
                if j == ne:
                    break
                if ret != prev:
                    acc = np.zeros(self.K, np.float32)
                prev = ret
                packed = int(sl[s, 1 + j, 0])
                w = np.array([sl[s, 1 + j, 1] & 0xffffffff], np.uint64).astype(np.uint32).view(np.float32)[0]
                f, l = packed % F, packed // F
                r = self.local[f][l].numpy().astype(np.float32)
                if mn[f]:
                    l2 = np.float32(0)
                    for x in r:
                        l2 = np.float32(l2 + np.float32(x * x))
                    nrm = np.sqrt(l2) if l2 > 0 else l2
                    r = (r * np.float32(mn[f])) / np.float32(max(nrm, np.float32(mn[f])))
                acc = (acc + r * w).astype(np.float32)
        if stat is not None:
            de = max(int(sl[s, 0, 1] & 0xffffffff) for s in range(P))
            db = max(int(sl[s, 0, 1] >> 32) for s in range(P))
            stat.copy_(torch.tensor([int(de > cap_e or db > cap_b), de, db]))

    def bags_combine(self, back, cap_b, pos, mask, denom, B, combiner, out, fm=None):
        F, P, K = self.F, self.P, self.K
        cb_ = self._codes(combiner)
        bk, ps, mk, dn = back.numpy(), pos.numpy(), mask.numpy(), denom.numpy()
        o_ = out.numpy()
        for b in range(B):
            for f in range(F):
                g = b * F + f
                m = int(mk[g]) & ((1 << 64) - 1)
                acc = np.zeros(K, np.float32)
                for o in range(P):
                    if (m >> o) & 1 and ps[g * P + o] >= 0:
                        acc = (acc + bk[ps[g * P + o]]).astype(np.float32)
                if m and cb_[f] != 0:
                    acc = (acc / dn[g]).astype(np.float32)
                o_[b, f * K:(f + 1) * K] = acc
        if fm is not None:
            e = o_.reshape(-1, F, K).astype(np.float64)
            fm.copy_(torch.from_numpy((0.5 * ((e.sum(1) ** 2) - (e ** 2).sum(1)).sum(1)).astype(np.float32)[:, None]))

    # ---- their backward ----
    def bags_grad(self, g, cap_b, pos, mask, denom, B, combiner, send):
        F, P, K = self.F, self.P, self.K
        comb = self._codes(combiner)
        gg, ps, mk, dn, sd = g.numpy(), pos.numpy(), mask.numpy(), denom.numpy(), send.numpy()
        for b in range(B):
            for f in range(F):
                gi = b * F + f
                m = int(mk[gi]) & ((1 << 64) - 1)
                if not m:
                    continue
                v = gg[b, f * K:(f + 1) * K].astype(np.float32)
                if comb[f] != 0:
                    v = (v / dn[gi]).astype(np.float32)
                for o in range(P):
                    p = int(ps[gi * P + o])
                    if (m >> o) & 1 and 0 <= p < P * cap_b:
                        sd[p] = v

    def bags_adagrad(self, opt, recv, cap_e, cap_b, grad_rows, max_norm):
        F, P = self.F, self.P
        sl = recv.numpy().reshape(P, cap_e + 1, 2)
        gr = grad_rows.numpy().astype(np.float64)
        mn = per_slot(max_norm, F)
        ent = []
        for s in range(P):
            ne = int(sl[s, 0, 0] & 0xffffffff)
            rec = sl[s, 1:1 + ne]
            packed = rec[:, 0]
            ret = rec[:, 1] >> 32
            w = (rec[:, 1] & 0xffffffff).astype(np.uint32).view(np.float32).astype(np.float64)
            ok = (packed >= 0) & (ret >= 0) & (ret < cap_b)
            ent.append((packed[ok], ret[ok] + s * cap_b, w[ok]))
        packed, gidx, w = (np.concatenate([e[c] for e in ent]) for c in range(3))
        for f in range(F):
            sel = (packed % F == f) & (packed // F < self.local[f].shape[0])
            rows_all = packed[sel] // F
            G = np.zeros(tuple(self.local[f].shape))
            np.add.at(G, rows_all, w[sel][:, None] * gr[gidx[sel]])
            rows = np.unique(rows_all)
            g = G[rows]
            if mn[f] and len(rows):                         # clip_by_norm's derivative at the pre-update row
                r = self.local[f].numpy().astype(np.float64)[rows]
                n = np.sqrt((r * r).sum(1, keepdims=True))
                gc = mn[f] * (g / np.maximum(n, 1e-30) - r * ((r * g).sum(1, keepdims=True) / np.maximum(n, 1e-30) ** 3))
                g = np.where(n > mn[f], gc, g)
            self._adagrad(opt, f, rows, g)
