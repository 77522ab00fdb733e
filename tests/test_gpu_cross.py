"""crossed_column on the GPU: the one-hot and ragged cross kernels, the device fingerprint of byte strings, a graph replay, and the models
that take a crossed column (wide & deep ESMM, DCN, the sharded DCN trainer) against twins fed the stand-in's ids through an identity
column.  Reference: tests/cross_standin.py.  Every comparison is bit for bit; there is no tolerance in this file."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cross_standin as S

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
SPECIALS = [0, -1, I64.max, I64.min]
BUCKETS = [1, 2, 128, (1 << 31) + 11, (1 << 62) + 57]          # the large ones catch a signed or 32-bit modulo


def _columns(rng, B, nk):
    """nk random int64 columns [B] over the full range; the special values 0, -1, 2^63-1, -2^63 land in the first rows, shifted per key."""
    cols = rng.integers(I64.min, I64.max, size=(nk, B), dtype=np.int64, endpoint=True)
    for k in range(nk):
        for j, v in enumerate(SPECIALS):
            cols[k, (j + k) % B] = v
    return cols


def _raw(cols, hash_key=S.HASH_KEY):
    """The chain's 64-bit value per sample (the id before the modulo), as Python ints."""
    return [S.cross_id(row, 1 << 64, hash_key) for row in zip(*cols.tolist())]


def _ids(raw, nb):
    return np.array([h % nb for h in raw], dtype=np.uint64).astype(np.int64)


def _sources(cols, strided):
    """The columns as device vectors: separate tensors, or the strided columns of one [B, F] matrix with a spare column in between."""
    nk, B = cols.shape
    if not strided:
        return [torch.from_numpy(cols[k].copy()).cuda() for k in range(nk)]
    mat = torch.zeros((B, 2 * nk + 1), dtype=torch.int64).cuda()
    mat[:, 1::2][:, :nk] = torch.from_numpy(cols.T.copy()).cuda()
    return [mat[:, 1 + 2 * k] for k in range(nk)]


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("nk", [2, 3, 8])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000])
def test_onehot_cross(built_lib, B, nk, strided):
    from dir_amd import ops
    rng = np.random.default_rng(1000 * B + 10 * nk + strided)
    cols = _columns(rng, B, nk)
    src = _sources(cols, strided)
    raw = _raw(cols)
    for nb in BUCKETS:
        got = ops.cross_hash(src, [(list(range(nk)), nb)])
        assert got.shape == (1, B) and got.dtype == torch.int64
        assert np.array_equal(got[0].cpu().numpy(), _ids(raw, nb)), (B, nk, nb)
    if B == 65:      # the hashing order is the order of the key list
        rev = ops.cross_hash(src, [(list(range(nk))[::-1], 1 << 62)])
        assert np.array_equal(rev[0].cpu().numpy(), _ids(_raw(cols[::-1]), 1 << 62))
        assert not np.array_equal(rev[0].cpu().numpy(), _ids(raw, 1 << 62))


def test_onehot_cross_hash_key_and_argument_errors(built_lib):
    from dir_amd import ops
    rng = np.random.default_rng(8)
    cols = _columns(rng, 65, 9)
    src = _sources(cols, False)
    for hk in (0x1234, 0, (1 << 64) - 1):
        got = ops.cross_hash(src[:3], [([0, 1, 2], 1000003, hk)])
        assert np.array_equal(got[0].cpu().numpy(), _ids(_raw(cols[:3], hk), 1000003)), hk
    assert int(ops.cross_hash([torch.tensor([3]).cuda(), torch.tensor([7]).cuda()], [([0, 1], 128, 0x1234)])[0, 0]) == 0xccdb65cdd3bf4aae % 128
    assert int(ops.cross_hash([torch.tensor([3]).cuda(), torch.tensor([7]).cuda()], [([0, 1], 128)])[0, 0]) == 41
    # nine keys: refused by ops, and an argument error at the ABI itself
    with pytest.raises(ValueError):
        ops.cross_hash(src, [(list(range(9)), 128)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cross_hash([s.cpu() for s in src[:2]], [([0, 1], 128)])
    out = torch.full((17, 65), -7, dtype=torch.int64).cuda()

    def raw_call(counts, n_src=9):
        flat = [k % n_src for c in counts for k in range(c)]
        nx = len(counts)
        return built_lib.dir_cross_onehot_i64((ctypes.c_void_p * 9)(*[s.data_ptr() for s in src]), (ctypes.c_int64 * 9)(*[1] * 9), n_src,
                                              (ctypes.c_int32 * len(flat))(*flat), (ctypes.c_int32 * nx)(*counts),
                                              (ctypes.c_uint64 * nx)(*[S.HASH_KEY] * nx), (ctypes.c_int64 * nx)(*[128] * nx), nx, 65,
                                              ctypes.c_void_p(out.data_ptr()), ops._stream())

    assert raw_call([9]) == -1 and b"9 keys" in built_lib.dir_last_error()
    assert raw_call([1]) == -1 and b"1 keys" in built_lib.dir_last_error()
    assert raw_call([2] * 17) == -1 and b"nx=17" in built_lib.dir_last_error()
    assert raw_call([2], n_src=33) == -1 and b"n_src=33" in built_lib.dir_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    assert raw_call([8]) == 0
    assert np.array_equal(out[0].cpu().numpy(), _ids(_raw(cols[:8]), 128)) and bool((out[1:] == -7).all())


@pytest.mark.parametrize("B", [65, 1000])
def test_several_crosses_in_one_launch(built_lib, B, monkeypatch):
    from dir_amd import _lib, ops
    rng = np.random.default_rng(B)
    cols = _columns(rng, B, 40)
    src = _sources(cols[:6], True) + _sources(cols[6:], False)
    launches = []
    lib = _lib.load()
    real = lib.dir_cross_onehot_i64
    monkeypatch.setattr(lib, "dir_cross_onehot_i64", lambda *a: (launches.append(a[7]), real(*a))[1])

    def check(crosses, want_launches):
        del launches[:]
        got = ops.cross_hash(src, crosses)
        assert launches == want_launches, launches
        assert got.shape == (len(crosses), B) and got.is_contiguous()
        del launches[:]
        for x, c in enumerate(crosses):
            single = ops.cross_hash(src, [c])
            assert torch.equal(got[x], single[0]), x
            hk = c[2] if len(c) > 2 else S.HASH_KEY
            assert np.array_equal(single[0].cpu().numpy(), _ids(_raw(cols[list(c[0])], hk), c[1])), x
        assert launches == [1] * len(crosses)

    # NX = 3 sharing source columns (0 and 2 are used twice, in different positions)
    check([([0, 2], 128), ([2, 7, 0], 1000003, 0x1234), ([1, 2], (1 << 62) + 57)], [3])
    # NX = 16, 2..8 keys each, every bucket size
    sixteen = [([int(k) for k in rng.choice(12, size=2 + x % 7, replace=False)], BUCKETS[x % 5], 77 + x) for x in range(16)]
    check(sixteen, [16])
    if B == 65:
        # more than one launch can hold: 20 crosses -> 16 + 4; 6 crosses over 40 distinct sources -> 4 + 2 (32 sources per launch)
        check(sixteen + sixteen[:4], [16, 4])
        check([(list(range(8 * x, 8 * x + 8)) if x < 5 else [0, 39], 128) for x in range(6)], [4, 2])


def test_collect_ids_forms_crossed_columns_in_one_launch(built_lib, monkeypatch):
    """Three crossed columns of one call: one launch, and the [B, 3] ids collect_ids returns ARE that launch's [3, B] output (no stack)."""
    from dir_amd import _input, feature_column as fc, ops
    rng = np.random.default_rng(4)
    B = 257
    a, b, c = _columns(rng, B, 3)
    feats = {"a": torch.from_numpy(a).cuda(), "b": torch.from_numpy(b).cuda(), "c": torch.from_numpy(c).cuda()}
    cols = [fc.crossed_column(["a", "b"], 128), fc.crossed_column(["c", "a", "b"], 1000), fc.crossed_column(["b", "c"], 50, hash_key=9)]
    made = []
    real = ops.cross_hash
    monkeypatch.setattr(ops, "cross_hash", lambda *args, **kw: (made.append(real(*args, **kw)), made[-1])[1])
    kind, ids = _input.collect_ids(cols, feats, torch.device("cuda"))
    _input.raise_pending(block=True)
    assert kind == "onehot" and len(made) == 1
    mat = made[0]
    assert len(mat.shape) == 2 and tuple(mat.shape) == (3, B)
    assert ids.shape == (B, 3) and ids.stride() == (1, B)
    assert ids.data_ptr() == mat.data_ptr() and ids.untyped_storage().data_ptr() == mat.untyped_storage().data_ptr()
    assert ids._base is mat
    want = np.stack([S.cross_onehot([a, b], 128), S.cross_onehot([c, a, b], 1000), S.cross_onehot([b, c], 50, 9)], axis=1)
    assert np.array_equal(ids.cpu().numpy(), want)
    # each column on its own gives the same ids; a model over embedding wrappers sees the same columns
    for j, col in enumerate(cols):
        assert np.array_equal(col.ids(feats, torch.device("cuda")).cpu().numpy(), want[:, j])
    # mixed with an identity column nothing changes for that column: the ids are stacked as before
    ident = fc.categorical_column_with_identity("a", 1 << 62, default_value=0)
    kind, ids2 = _input.collect_ids([cols[0], ident], feats, torch.device("cuda"))
    _input.raise_pending(block=True)
    assert kind == "onehot" and np.array_equal(ids2[:, 0].cpu().numpy(), want[:, 0])
    assert np.array_equal(ids2[:, 1].cpu().numpy(), np.where((a < 0) | (a >= 1 << 62), 0, a))


# ---- ragged ------------------------------------------------------------------------------------------------------------------------------
def _ragged(rng, lens):
    lens = np.asarray(lens, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    vals = rng.integers(I64.min, I64.max, size=int(offs[-1]), dtype=np.int64, endpoint=True)
    vals[:min(4, len(vals))] = SPECIALS[:min(4, len(vals))]
    return vals, offs


def _ragged_cases():
    rng = np.random.default_rng(21)
    cases = {}
    # B = 1: ragged, one-hot, ragged -> 2 * 1 * 3
    cases["b1"] = [_ragged(rng, [2]), rng.integers(-9, 9, size=1), _ragged(rng, [3])]
    # B = 5: products 2*3, 0 (first ragged key empty), 0 (second empty), 1*7*2, 1
    cases["b5"] = [rng.integers(I64.min, I64.max, size=5), _ragged(rng, [2, 0, 1, 7, 1]), _ragged(rng, [3, 1, 0, 2, 1])]
    # B = 5, all rows empty: a cross without entries
    cases["empty"] = [_ragged(rng, [0] * 5), _ragged(rng, [0, 2, 0, 1, 0])]
    # B = 257: lengths 0..3, a one-hot key in the middle, four keys
    cases["b257"] = [_ragged(rng, rng.integers(0, 4, size=257)), rng.integers(I64.min, I64.max, size=257),
                     _ragged(rng, rng.integers(0, 4, size=257)), _ragged(rng, rng.integers(1, 3, size=257))]
    # B = 257: one row of 40 * 50 entries among one-entry rows
    l0, l1 = np.ones(257, dtype=np.int64), np.ones(257, dtype=np.int64)
    l0[100], l1[100] = 40, 50
    cases["hot"] = [_ragged(rng, l0), _ragged(rng, l1)]
    return cases


_RAGGED = _ragged_cases()


def _dev_keys(keys, strided_onehot=False):
    out = []
    for k in keys:
        if isinstance(k, tuple):
            out.append((torch.from_numpy(k[0]).cuda(), torch.from_numpy(k[1]).cuda()))
        elif strided_onehot:
            m = torch.zeros((len(k), 3), dtype=torch.int64).cuda()
            m[:, 1] = torch.from_numpy(np.asarray(k, dtype=np.int64)).cuda()
            out.append(m[:, 1])
        else:
            out.append(torch.from_numpy(np.asarray(k, dtype=np.int64)).cuda())
    return out


@pytest.mark.parametrize("name", sorted(_RAGGED))
@pytest.mark.parametrize("nb", [128, (1 << 62) + 57])
def test_ragged_cross(built_lib, name, nb):
    from dir_amd import ops
    keys = _RAGGED[name]
    want_ids, want_offs = S.cross_ragged(keys, nb)
    if name == "b5":
        assert np.diff(want_offs).tolist() == [6, 0, 0, 14, 1]
    if name == "hot":
        assert int(np.diff(want_offs)[100]) == 2000 and len(want_ids) == 2256
    vals, offs = ops.cross_hash_ragged(_dev_keys(keys, strided_onehot=(nb == 128)), nb)
    assert np.array_equal(offs.cpu().numpy(), want_offs)
    assert vals.dtype == torch.int64 and np.array_equal(vals.cpu().numpy(), want_ids)
    hk = 0x1234
    vals, offs = ops.cross_hash_ragged(_dev_keys(keys), nb, hash_key=hk)
    w2, _ = S.cross_ragged(keys, nb, hk)
    assert np.array_equal(vals.cpu().numpy(), w2)


def test_ragged_fill_checks_the_capacity(built_lib):
    """A fill told a capacity that is not the offsets' total reports it in the status word and writes NOTHING: neither the guard words
    behind the output nor the output itself."""
    from dir_amd import ops
    keys = _RAGGED["b5"]
    want_ids, want_offs = S.cross_ragged(keys, 1000)
    total = len(want_ids)
    dkeys = _dev_keys(keys)
    GUARD = -0x5A5A5A5A5A5A5A5B
    for cap in (total - 1, total + 2, 0):
        buf = torch.full((total + 8,), GUARD, dtype=torch.int64).cuda()
        vals, offs, status = ops.cross_hash_ragged(dkeys, 1000, capacity=cap, out=buf, return_status=True)
        assert int(status[0]) == 1, cap
        assert bool((buf == GUARD).all()), cap
        assert np.array_equal(offs.cpu().numpy(), want_offs)
    buf = torch.full((total + 8,), GUARD, dtype=torch.int64).cuda()
    vals, offs, status = ops.cross_hash_ragged(dkeys, 1000, capacity=total, out=buf, return_status=True)
    assert int(status[0]) == 0 and vals.data_ptr() == buf.data_ptr()
    assert np.array_equal(buf[:total].cpu().numpy(), want_ids) and bool((buf[total:] == GUARD).all())
    with pytest.raises(ValueError):
        ops.cross_hash_ragged(dkeys[:1], 1000)
    with pytest.raises(ValueError):
        ops.cross_hash_ragged(dkeys, 0)


def test_crossed_column_over_ragged_features(built_lib):
    """fc.crossed_column with a Ragged feature and a vocabulary column as keys: (values, offsets, None), the column's -1 crossed like any id."""
    from dir_amd import feature_column as fc
    rng = np.random.default_rng(2)
    tags_v, tags_o = _ragged(rng, [2, 0, 3, 1])
    rel = ["a", "zz", "b", "a"]
    relc = fc.categorical_column_with_vocabulary_list("rel", ["a", "b"])
    col = fc.crossed_column([relc, "tags", "city"], 97)
    city = ["Oslo", "", "Lima", "Oslo"]
    feats = {"rel": rel, "tags": fc.Ragged(torch.from_numpy(tags_v), torch.from_numpy(tags_o)), "city": city}
    vals, offs, w = col.ids(feats, torch.device("cuda"))
    assert w is None
    want, want_offs = S.cross_ragged([[0, -1, 1, 0], (tags_v, tags_o), city], 97)
    assert np.array_equal(offs.cpu().numpy(), want_offs) and np.array_equal(vals.cpu().numpy(), want)


# ---- strings -----------------------------------------------------------------------------------------------------------------------------
def test_device_fingerprint_of_byte_strings(built_lib):
    """Every length from 0 to 100 (FarmHash's <= 16, 17-32, 33-64 and > 64 byte branches), and a few longer ones."""
    from dir_amd import ops
    rng = np.random.default_rng(6)
    strs = [bytes(rng.integers(0, 256, size=n, dtype=np.uint8).tolist()) for n in list(range(0, 101)) + [127, 128, 129, 1000]]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in strs])]).astype(np.int64)
    buf = torch.from_numpy(np.frombuffer(b"".join(strs), dtype=np.uint8).copy()).cuda()
    got = ops.fingerprint64_bytes(buf, torch.from_numpy(offs).cuda()).cpu()
    host = ops.fingerprint64_strings(strs)
    assert torch.equal(got, host)
    for s, g in zip(strs, got.tolist()):
        assert g & S.M64 == ops.fingerprint64(s) == S.contribution(s), len(s)
    with pytest.raises(TypeError):
        ops.fingerprint64_bytes(buf.cpu(), torch.from_numpy(offs).cuda())


def test_crossed_column_over_string_features(built_lib):
    from dir_amd import feature_column as fc
    wc = ["Private", "?", "", "State-gov", "Private"]
    ed = ["Bachelors", "HS-grad", "Bachelors", "", "Bachelors"]
    age = torch.tensor([39, -1, 0, 50, 39])
    col = fc.crossed_column(["workclass", "education"], 128)
    got = col.ids({"workclass": wc, "education": ed}, torch.device("cuda"))
    assert np.array_equal(got.cpu().numpy(), S.cross_onehot([wc, ed], 128))
    assert got[0] == got[4]
    col3 = fc.crossed_column([col, "age"], 1000)               # nested: workclass, education, age; the integer is NOT hashed first
    got = col3.ids({"workclass": wc, "education": ed, "age": age.cuda()}, torch.device("cuda"))
    assert np.array_equal(got.cpu().numpy(), S.cross_onehot([wc, ed, age.tolist()], 1000))


# ---- graph -------------------------------------------------------------------------------------------------------------------------------
def test_onehot_cross_graph_replay(built_lib):
    from dir_amd import ops
    rng = np.random.default_rng(12)
    B = 1000
    cols = _columns(rng, B, 3)
    mat = torch.from_numpy(cols.T.copy()).cuda()
    src = [mat[:, k] for k in range(3)]
    crosses = [([0, 1], 128), ([2, 0, 1], (1 << 31) + 11, 5)]
    out = torch.empty((2, B), dtype=torch.int64).cuda()
    ops.cross_hash(src, crosses, out=out)                      # one eager call first
    first = out.clone()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            ops.cross_hash(src, crosses, out=out)
    torch.cuda.current_stream().wait_stream(side)
    new = _columns(np.random.default_rng(13), B, 3)
    mat.copy_(torch.from_numpy(new.T.copy()).cuda())           # new values in the same buffers
    out.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager = ops.cross_hash(src, crosses)
    assert torch.equal(replayed, eager) and not torch.equal(replayed, first)
    assert np.array_equal(replayed[1].cpu().numpy(), _ids(_raw(new[[2, 0, 1]], 5), (1 << 31) + 11))


# ---- models ------------------------------------------------------------------------------------------------------------------------------
EDUCATION = ['Bachelors', 'HS-grad', '11th', 'Masters', '9th', 'Some-college', 'Assoc-acdm', 'Assoc-voc', '7th-8th', 'Doctorate',
             'Prof-school', '5th-6th', '10th', '1st-4th', 'Preschool', '12th']
MARITAL = ['Married-civ-spouse', 'Divorced', 'Married-spouse-absent', 'Never-married', 'Separated', 'Married-AF-spouse', 'Widowed']
RELATIONSHIP = ['Husband', 'Not-in-family', 'Wife', 'Own-child', 'Unmarried', 'Other-relative']
WORKCLASS = ['Self-emp-not-inc', 'Private', 'State-gov', 'Federal-gov', 'Local-gov', '?', 'Self-emp-inc', 'Without-pay', 'Never-worked']
NUMERIC = ['age', 'education_num', 'capital_gain', 'capital_loss', 'hours_per_week']
WIDE = "education_X_workclass"


def _census_columns(wide):
    """The reference's column set (models/ESMM/train.py:56-112), restated; `wide`: the wide part's one column."""
    from dir_amd import feature_column as fc
    vocab = fc.categorical_column_with_vocabulary_list
    deep = [fc.numeric_column(k) for k in NUMERIC]
    deep += [fc.indicator_column(vocab("workclass", WORKCLASS)), fc.indicator_column(vocab("education", EDUCATION)),
             fc.indicator_column(vocab("marital_status", MARITAL)), fc.indicator_column(vocab("relationship", RELATIONSHIP)),
             fc.indicator_column(vocab("income_bracket", ["<=50K", ">50k"])),
             fc.embedding_column(fc.categorical_column_with_hash_bucket("occupation", hash_bucket_size=1000), dimension=8)]
    return [wide], deep


def _census_features(rng, B):
    pick = lambda names: [names[i] for i in rng.integers(0, len(names), size=B)]
    f = {k: torch.from_numpy(rng.uniform(0, 1, B).astype(np.float32)).cuda() for k in NUMERIC}
    f.update(workclass=pick(WORKCLASS + ["Unknown"]), education=pick(EDUCATION), marital_status=pick(MARITAL), relationship=pick(RELATIONSHIP),
             income_bracket=pick(["<=50K", ">50k"]), occupation=pick(["Sales", "Tech-support", "?", "Exec-managerial", "Craft-repair"]))
    return f


def test_esmm_wide_deep_with_the_reference_columns(built_lib):
    """ESMM_W_D whose wide part is crossed_column(["workclass", "education"], 128) against the same model whose wide column is an identity
    column of 128 buckets fed the stand-in's ids: predict bitwise equal, and after one training step with the fused sparse FTRL on the
    linear weights bitwise the same linear weights."""
    from dir_amd import feature_column as fc, ops
    from dir_amd.esmm import ESMM_W_D
    rng = np.random.default_rng(17)
    B = 300
    feats = _census_features(rng, B)
    twin_feats = dict(feats)
    twin_feats[WIDE] = torch.from_numpy(S.cross_onehot([feats["workclass"], feats["education"]], 128)).cuda()
    crossed = fc.crossed_column(["workclass", "education"], 128)
    assert crossed.name == WIDE

    def make(wide):
        torch.manual_seed(3)
        lin, deep = _census_columns(wide)
        return ESMM_W_D(linear_feature_columns=lin, dnn_feature_columns=deep, dnn_hidden_units=[64, 64, 64]).cuda()

    model, twin = make(crossed), make(fc.categorical_column_with_identity(WIDE, 128))
    with torch.no_grad():
        for sub in (model.ctr_model, model.cvr_model):
            for w in sub.linear.weights:
                w.normal_(0, 0.1)
            sub.linear.bias.fill_(0.3)
    twin.load_state_dict(model.state_dict())
    with torch.no_grad():
        got, want = model.predict(feats), twin.predict(twin_feats)
    assert sorted(got) == sorted(want)
    for k in got:
        assert torch.equal(got[k], want[k]), k
    assert float(got["ctr_logits"].std()) > 0
    labels = {"click_label": torch.from_numpy((rng.random(B) < 0.3).astype(np.float32)).cuda(),
              "convert_label": torch.from_numpy((rng.random(B) < 0.1).astype(np.float32)).cuda()}
    before = [w.detach().clone() for w in model.ctr_model.linear.weights]
    for m, f in ((model, feats), (twin, twin_feats)):
        m.train()
        opts = [ops.SparseFtrl(sub.linear._tableset(), 0.2, l1=0.001).attach() for sub in (m.ctr_model, m.cvr_model)]
        loss, _ = m.get_loss(f, labels, m(f))
        loss.backward()
        assert bool(torch.isfinite(loss)) and len(opts) == 2
    torch.cuda.synchronize()
    for a, b in ((model.ctr_model, twin.ctr_model), (model.cvr_model, twin.cvr_model)):
        for wa, wb in zip(a.linear.weights, b.linear.weights):
            assert wa.shape == (128,) and torch.equal(wa.detach(), wb.detach())
    assert not torch.equal(before[0], model.ctr_model.linear.weights[0].detach()), "the step must have moved the wide weights"


def _dcn_pair(extra_cols, seed=5, **kw):
    """A DeepCrossNetwork over a crossed column's wrappers and its twin over an identity column of the same NAME (so that the input layer
    sorts both the same way) -> (model, twin)."""
    from dir_amd import feature_column as fc
    from dir_amd.dcn import DeepCrossNetwork
    out = []
    for cat in (fc.crossed_column(["workclass", "education"], 128), fc.categorical_column_with_identity(WIDE, 128)):
        torch.manual_seed(seed)
        out.append(DeepCrossNetwork(columns=extra_cols(cat), cross_layer_num=2, dnn_hidden_units=[32, 16], batch_norm=False, **kw).cuda())
    out[1].load_state_dict(out[0].state_dict())
    return out


def test_dcn_with_crossed_embedding_and_indicator(built_lib):
    from dir_amd import feature_column as fc
    rng = np.random.default_rng(19)
    B = 130
    feats = _census_features(rng, B)
    feats["item"] = torch.from_numpy(rng.integers(0, 50, size=B)).cuda()
    twin_feats = dict(feats)
    twin_feats[WIDE] = torch.from_numpy(S.cross_onehot([feats["workclass"], feats["education"]], 128)).cuda()
    item = fc.categorical_column_with_identity("item", 50)
    model, twin = _dcn_pair(lambda cat: [fc.numeric_column("age"), fc.numeric_column("hours_per_week"), fc.embedding_column(item, 8),
                                         fc.embedding_column(cat, 8), fc.indicator_column(cat)])
    names = [c.name for c in model.input_layer.columns]
    assert names == ["age", WIDE + "_embedding", WIDE + "_indicator", "hours_per_week", "item_embedding"] == sorted(names)
    assert names == [c.name for c in twin.input_layer.columns]
    model.eval(), twin.eval()
    with torch.no_grad():
        x0, t0 = model.input_layer(feats), twin.input_layer(twin_feats)
        got, want = model.predict(feats), twin.predict(twin_feats)
    assert x0.shape == (B, 1 + 8 + 128 + 1 + 8) and torch.equal(x0, t0)
    ids = twin_feats[WIDE]
    assert torch.equal(x0[:, 9:137].argmax(dim=1), ids) and bool((x0[:, 9:137].sum(dim=1) == 1).all())
    for k in got:
        assert torch.equal(got[k], want[k]), k
    # the differentiable path's forward
    model.train(), twin.train()
    la, lb = model(feats), twin(twin_feats)
    assert la.requires_grad and torch.equal(la.detach(), lb.detach())


def test_sharded_dcn_trainer_world1_with_a_crossed_column(built_lib):
    """ShardedDCNTrainer at world size 1 over a features dict that holds the crossed column's raw keys: predict equals the single-GPU
    model's, and the trainer whose crossed column is replaced by its identity twin."""
    from dir_amd import feature_column as fc
    from dir_amd.shard import ShardedDCNTrainer
    rng = np.random.default_rng(23)
    B = 256
    feats = _census_features(rng, B)
    for i in range(3):
        feats["C%02d" % i] = torch.from_numpy(rng.integers(0, 300, size=B)).cuda()
    twin_feats = dict(feats)
    twin_feats[WIDE] = torch.from_numpy(S.cross_onehot([feats["workclass"], feats["education"]], 128)).cuda()
    nums = NUMERIC[:4]          # 4 x 16 + 4 columns: a multiple of 4, the row layout both paths share
    model, twin = _dcn_pair(lambda cat: [fc.embedding_column(fc.categorical_column_with_identity("C%02d" % i, 300), 16) for i in range(3)] +
                            [fc.embedding_column(cat, 16)] + [fc.numeric_column(n) for n in nums], optimizer="Adam")
    outs = []
    for m, f in ((model, feats), (twin, twin_feats)):
        tables = ShardedDCNTrainer.tables_from_model(m)
        tr = ShardedDCNTrainer(m, tables)
        outs.append(tr.predict(f))
    m_eval = model.eval()
    with torch.no_grad():
        single = m_eval.predict(feats)
    for k in ("logits", "logistic", "probabilities"):
        print(k, "sharded vs twin", float((outs[0][k] - outs[1][k]).abs().max()), "sharded vs single GPU", float((outs[0][k] - single[k]).abs().max()))
    for k in ("logits", "logistic", "probabilities", "class_ids"):
        assert torch.equal(outs[0][k], outs[1][k]), k
        assert torch.equal(outs[0][k], single[k]), k
    assert float(single["logits"].std()) > 0
