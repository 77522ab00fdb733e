"""The first-order term over row-sharded multi-hot bags, for the tests: the NumPy stand-ins of its four backend steps (a subclass of
tests.shard_standin.NumpyBackend: bags_linear_pool, bags_linear_combine, bags_linear_grad, bags_ftrl -- reading and writing the kernels'
buffers in the kernels' formats and order, include/dir_hip.h: dir_shard_bags_linear_pool_f32 ... dir_sparse_ftrl_rows_sorted_bags_f32) and
the float64 reference over the FULL weights and the GLOBAL bags that the gloo and the GPU tests share."""
import numpy as np
import torch

from tests.shard_standin import _CODES, NumpyBackend

LIN_COMBINERS = ("sum", "mean", "sqrtn")


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------
def lin_entries(bags, vocab, lin_comb, prune):
    """The live entries of the bags with the coefficient each contributes to its sample's term: per slot f -> (sample index [n_f], ids [n_f],
    coef [n_f] = w_e * c_bag), c_bag = 1 (sum), 1 / sum w (mean; 1 / count without weights), 1 / sqrt(sum w^2) (sqrtn; 1 / sqrt(count)).
    Liveness is the lookup's: id inside [0, vocab_f), weight > 0 under prune."""
    out = []
    for f, V in enumerate(vocab):
        bi, ids, coef = [], [], []
        for b, row in enumerate(bags):
            i_, w_ = row[f]
            live = [(int(i), 1.0 if w_ is None else float(w_[j])) for j, i in enumerate(i_)
                    if 0 <= i < V and not (prune and w_ is not None and not float(w_[j]) > 0)]
            if not live:
                continue
            ws = np.array([w for _, w in live])
            if lin_comb == "mean":
                den = ws.sum() if w_ is not None else float(len(live))
            elif lin_comb == "sqrtn":
                den = np.sqrt((ws * ws).sum()) if w_ is not None else np.sqrt(float(len(live)))
            else:
                den = 1.0
            for (i, w) in live:
                bi.append(b)
                ids.append(i)
                coef.append(w / den)
        out.append((np.asarray(bi, np.int64), np.asarray(ids, np.int64), np.asarray(coef, np.float64)))
    return out


def lin_forward64(W, entries, B):
    """lin [B] in float64: W[f] = the full first-order weights of slot f ([vocab_f] or [vocab_f, 1]), entries = lin_entries(...)."""
    lin = np.zeros(B)
    for f, (bi, ids, coef) in enumerate(entries):
        np.add.at(lin, bi, coef * np.asarray(W[f], np.float64).reshape(-1)[ids])
    return lin


def lin_ftrl64(w, n, z, entries, dlin, lr, l1, l2):
    """One FTRL step of the full first-order weights (float64 [vocab_f, 1] arrays, in place) with the per-entry gradients coef * d lin[b]:
    oracle.np_ref.sparse_ftrl_step per slot (all entries of a row are summed before n, z and w move)."""
    from oracle import np_ref as R
    d = np.asarray(dlin, np.float64).reshape(-1)
    for f, (bi, ids, coef) in enumerate(entries):
        if len(ids):
            R.sparse_ftrl_step([w[f]], [n[f]], [z[f]], ids.reshape(-1, 1), (coef * d[bi]).reshape(-1, 1), lr, l1, l2)


# ---- NumPy stand-ins of the four backend steps ---------------------------------------------------------------------------------------
def _records(recv, P, cap_e):
    """The received slabs as (slab, header count, packed [ne], weight fp32 [ne], return position [ne]) per sender."""
    sl = recv.numpy().reshape(P, cap_e + 1, 2)
    for s in range(P):
        ne = int(sl[s, 0, 0] & 0xffffffff)
        rec = sl[s, 1:1 + ne]
        yield s, rec[:, 0], (rec[:, 1] & 0xffffffff).astype(np.uint32).view(np.float32), rec[:, 1] >> 32


class BagsLinearBackend(NumpyBackend):
    def bags_linear_pool(self, recv, cap_e, cap_b, out):
        F, P = self.F, self.P
        o = out.numpy()
        o[:P * cap_b] = 0.0                                # every word is written
        for s, packed, w, ret in _records(recv, P, cap_e):
            j, ne = 0, len(packed)
            while j < ne:                                  # one run per return position, fp32 in entry order from 0
                r, acc = int(ret[j]), np.float32(0)
                while j < ne and int(ret[j]) == r:
                    p = int(packed[j])
                    f, l = p % F, p // F
                    if p >= 0 and 0 <= r < cap_b and l < self.lin[f].shape[0]:
                        acc = np.float32(acc + np.float32(w[j] * self.lin[f].numpy()[l, 0]))
                    j += 1
                if 0 <= r < cap_b:
                    o[s * cap_b + r] = acc

    def _lden(self, vals, offs, wts, bag, f, code, prune):
        wsum, w2sum, n = np.float32(0), np.float32(0), 0
        for e in range(offs[bag], offs[bag + 1]):
            w = np.float32(1) if wts is None else np.float32(wts[e])
            if vals[e] < 0 or vals[e] >= self.vocab[f] or (prune and not w > 0):
                continue
            wsum, w2sum, n = np.float32(wsum + w), np.float32(w2sum + np.float32(w * w)), n + 1
        if code == 1:
            return wsum if wts is not None else np.float32(n)
        return np.sqrt(w2sum) if wts is not None else np.sqrt(np.float32(n))

    def bags_linear_combine(self, lback, cap_b, pos, mask, values, offsets, weights, B, sb, sf, flags, combiner, lden, bias, out):
        F, P = self.F, self.P
        code = _CODES[combiner]
        lb, ps, mk = lback.numpy(), pos.numpy(), mask.numpy()
        vals, offs = values.numpy(), offsets.numpy()
        wts = None if weights is None else weights.numpy()
        prune = wts is not None and bool(flags & 1)
        res = np.zeros((B, 1), np.float32)
        for b in range(B):
            acc = np.float32(0)
            for f in range(F):
                g = b * F + f
                m = int(mk[g]) & ((1 << 64) - 1)
                v = np.float32(0)
                for o in range(P):
                    if (m >> o) & 1 and 0 <= ps[g * P + o] < P * cap_b:
                        v = np.float32(v + lb[ps[g * P + o]])
                if code:
                    lden.numpy()[g] = self._lden(vals, offs, wts, b * sb + f * sf, f, code, prune)
                    if m:
                        v = np.float32(v / lden.numpy()[g])
                acc = np.float32(acc + v)
            res[b, 0] = np.float32(acc + (np.float32(bias.numpy().reshape(-1)[0]) if bias is not None else np.float32(0)))
        out.copy_(torch.from_numpy(res))

    def bags_linear_grad(self, g, cap_b, pos, mask, lden, B, combiner, send):
        F, P = self.F, self.P
        code = _CODES[combiner]
        gg, ps, mk, sd = g.detach().numpy().reshape(-1), pos.numpy(), mask.numpy(), send.numpy()
        for b in range(B):
            for f in range(F):
                gi = b * F + f
                m = int(mk[gi]) & ((1 << 64) - 1)
                if not m:
                    continue
                d = np.float32(gg[b] / lden.numpy()[gi]) if code else np.float32(gg[b])
                for o in range(P):
                    p = int(ps[gi * P + o])
                    if (m >> o) & 1 and 0 <= p < P * cap_b:
                        sd[p] = d

    def bags_ftrl(self, recv, cap_e, cap_b, grad, lr, l1, l2, sorted_by=None):
        self.ftrl_calls += 1
        F, P = self.F, self.P
        gr = grad.numpy().astype(np.float64)
        gs = [np.zeros(r.shape[0]) for r in self.lin]
        hit = [np.zeros(r.shape[0], bool) for r in self.lin]
        for s, packed, w, ret in _records(recv, P, cap_e):
            for p, wj, r in zip(packed, w.astype(np.float64), ret):
                f, l = int(p) % F, int(p) // F
                if p >= 0 and 0 <= r < cap_b and l < self.lin[f].shape[0]:
                    gs[f][l] += wj * gr[s * cap_b + int(r)]        # ALL entries of a row are summed before n, z and w move
                    hit[f][l] = True
        for f in range(F):
            r, t = self.lin[f].numpy(), hit[f]
            r[t, 0], r[t, 1], r[t, 2] = self._ftrl(*(r[t, c].astype(np.float64) for c in range(3)), gs[f][t], lr, l1, l2)
