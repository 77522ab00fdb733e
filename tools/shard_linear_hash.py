"""tools/shard_linear_hash.py (GPU box): a seeded fingerprint of the sharded first-order term at world size 1, for comparing two commits bit
for bit.  Three trainers -- ShardedDeepFMTrainer(linear=) with dedup=False and dedup=True (units = 1), ShardedESMMTrainer on an ESMM_W_D
(units = 2) -- take three steps and one predict each; the embedding shards, the packed first-order rows (lin_rows: w, n, z of every
unit) and the logits are hashed (SHA-256 over the raw bytes).  Every case runs twice in one process: "stable" says whether the two runs
gave the same bytes, without which a difference between two commits means nothing.  Every batch draws each slot's ids without
repetition: the slab position of an entry is decided by the bucket pass's atomics, so the ORDER in which a row's entries are summed --
and with it the last bit of a sum of several -- may change from run to run at one commit (with Zipf batches in the dedup=True case the
two runs of one process disagreed, at the parent commit too); a row named once per batch gets that entry's gradient whatever the order.
One JSON line: {"cases": {name: hash}, "arrays": count, "stable": {name: bool}}.  Run it at both commits and compare the lines."""
import hashlib
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import dir_amd  # noqa: E402
from dir_amd import feature_column as fc  # noqa: E402
from dir_amd.shard import ShardedDeepFMTrainer, ShardedESMMTrainer, ShardedTables  # noqa: E402

dir_amd.load_library()
dev = torch.device("cuda", 0)
VOCAB, K, B, STEPS = [500, 1000, 7, 64], 16, 384, 3
F = len(VOCAB)
FTRL = dict(lr=0.15, l1=0.01, l2=0.02)


def ids_of(rng):
    cols = []
    for v in VOCAB:
        c = np.full(B, -1, np.int64)                         # ids < 0 are pruned: a small table gives what rows it has, once each
        k = min(B - B // 16, v)
        c[rng.permutation(B)[:k]] = rng.permutation(v)[:k]
        cols.append(c)
    return torch.from_numpy(np.stack(cols, axis=1).astype(np.int64)).to(dev)


class Digest:
    def __init__(self):
        self.h, self.n = hashlib.sha256(), 0

    def add(self, *tensors):
        for t in tensors:
            self.h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
            self.n += 1


def state(d, tables):
    d.add(*tables.local_tables)
    d.add(*tables.lin_rows)


def deepfm(dedup):
    from dir_amd.deepfm import DeepFM
    cats = [fc.categorical_column_with_identity("c%d" % i, v) for i, v in enumerate(VOCAB)]
    torch.manual_seed(7)
    m = DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K) for c in cats], dnn_hidden_units=[16, 16],
               fm_embedding_size=K)
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        for w in m.linear_weights:
            w.copy_(0.3 * torch.randn(w.shape, generator=g))
        m.linear_bias.fill_(0.05)
    m = m.to(dev)
    dense = [p for n, p in m.named_parameters() if not n.startswith(("embedding_weights", "linear_weights")) and n != "linear_bias"]
    tables = ShardedTables.from_full([p.detach().clone() for p in m.embedding_weights])
    tables.attach_linear_from_full([p.detach().clone() for p in m.linear_weights], 0.1)
    tr = ShardedDeepFMTrainer(m, tables, 0.05, torch.optim.SGD(dense, lr=0.01), linear=FTRL, dedup=dedup)
    rng = np.random.default_rng(21)
    d = Digest()
    for _ in range(STEPS):
        tr.step(ids_of(rng), torch.from_numpy(rng.integers(0, 2, size=(B, 1)).astype(np.float32)).to(dev))
        state(d, tables)
    d.add(tr.predict(ids_of(rng)))
    return d


def esmm():
    from dir_amd.esmm import ESMM_W_D
    cats = [fc.categorical_column_with_identity("c%d" % i, v) for i, v in enumerate(VOCAB)]
    torch.manual_seed(5)
    m = ESMM_W_D(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K) for c in cats], dnn_hidden_units=[16])
    with torch.no_grad():
        for sub in (m.ctr_model, m.cvr_model):
            for w in sub.linear.weights:
                w.copy_(0.3 * torch.randn(w.shape))
    m = m.to(dev)
    tables = ShardedESMMTrainer.tables_from_model(m)
    dense = [p for n, p in m.named_parameters() if "embedding_weights" not in n and ".linear." not in n]
    tr = ShardedESMMTrainer(m, tables, 0.05, torch.optim.SGD(dense, lr=0.01), linear=FTRL)
    rng = np.random.default_rng(43)
    d = Digest()
    for _ in range(STEPS):
        y = torch.from_numpy(rng.integers(0, 2, size=(B, 2)).astype(np.float32)).to(dev)
        wc = torch.from_numpy(rng.uniform(0.5, 2.0, size=(B, 1)).astype(np.float32)).to(dev)
        tr.step(ids_of(rng), y, wc, None)
        state(d, tables)
    d.add(*tr.predict(ids_of(rng)).values())                 # ctr, cvr and ctcvr logits
    return d


cases = {"deepfm_linear": lambda: deepfm(False), "deepfm_linear_dedup": lambda: deepfm(True), "esmm_w_d": esmm}
res, arrays, stable = {}, 0, {}
for name, fn in cases.items():
    a, b = fn(), fn()
    torch.cuda.synchronize()
    res[name] = a.h.hexdigest()
    arrays += a.n
    stable[name] = a.h.hexdigest() == b.h.hexdigest()
print(json.dumps({"cases": res, "arrays": arrays, "stable": stable}))
