"""CPU tests of crossed_column: the host entry of the hash the kernels chain, the host batch fingerprint, the constructor's rules, the
checkpoint name of a crossed linear column, and the stand-in's own product order.  Every comparison is bit for bit."""
import ctypes

import numpy as np
import pytest

from tests import cross_standin as S

KEY = 0xDECAFCAFFE
M64 = (1 << 64) - 1


def _raw_cat(lib):
    """dir_fingerprint_cat64 through raw ctypes (a handle of its own: nothing of the package's binding table is involved)."""
    import dir_amd
    raw = ctypes.CDLL(dir_amd.library_path())
    fn = raw.dir_fingerprint_cat64
    fn.restype, fn.argtypes = ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]
    return fn


def test_fingerprint_cat64_known_answers(built_lib):
    cat = _raw_cat(built_lib)
    assert cat(KEY, 0) == 0x1b107540f214cd46
    assert cat(KEY, 1) == 0xc82807364dd0cffc
    assert cat(0, 0) == 0x5825f5f3bd962979
    h = cat(cat(KEY, 3), 7)
    assert h == 0xf80ba4cd30a7bd29 and h % 128 == 41
    assert cat(cat(KEY, M64), 5) == 0x074f4692469f42f7
    h = cat(cat(cat(KEY, 1), 2), 3)
    assert h == 0x3799ea3692d74383 and h % 1000003 == 948881
    assert cat(cat(0x1234, 3), 7) == 0xccdb65cdd3bf4aae
    # the stand-in states the same formula
    assert S.cat64(S.cat64(KEY, 3), 7) == 0xf80ba4cd30a7bd29 and S.cross_id([3, 7], 128) == 41
    assert S.cross_id([1, 2, 3], 1000003) == 948881 and S.cross_id([-1, 5], 1 << 64) == 0x074f4692469f42f7


def test_fingerprint_cat64_matches_standin_on_random_pairs(built_lib):
    from dir_amd import ops
    cat = _raw_cat(built_lib)
    rng = np.random.default_rng(11)
    pairs = rng.integers(0, 1 << 64, size=(10000, 2), dtype=np.uint64)
    pairs[:4] = [[0, 0], [M64, M64], [0, M64], [1 << 63, 1]]
    for a, b in pairs.tolist():
        assert cat(a, b) == S.cat64(a, b), (a, b)
    assert ops.fingerprint_cat64(-1, 5) == S.cat64(M64, 5)          # the ops wrapper takes Python ints of either sign


def test_host_batch_fingerprint_equals_single_calls(built_lib):
    import torch
    from dir_amd import ops
    rng = np.random.default_rng(5)
    strs = [b"", b"a", "Private", "Bachelors", "Self-emp-not-inc", "éè"] + \
           [bytes(rng.integers(0, 256, size=n, dtype=np.uint8).tolist()) for n in (1, 7, 8, 16, 17, 32, 33, 64, 65, 200)]
    got = ops.fingerprint64_strings(strs)
    assert got.dtype == torch.int64 and got.device.type == "cpu" and got.shape == (len(strs),)
    for s, g in zip(strs, got.tolist()):
        assert g & M64 == ops.fingerprint64(s) == S.contribution(s), s
    assert ops.fingerprint64_strings([]).shape == (0,)


def test_crossed_column_constructor_rules(built_lib):
    from dir_amd import feature_column as fc
    with pytest.raises(ValueError):
        fc.crossed_column(["workclass"], 128)
    with pytest.raises(ValueError):
        fc.crossed_column([], 128)
    with pytest.raises(ValueError):
        fc.crossed_column(["workclass", "education"], 0)
    with pytest.raises(ValueError, match="hash_bucket"):
        fc.crossed_column(["workclass", fc.categorical_column_with_hash_bucket("education", 100)], 128)
    ident = fc.categorical_column_with_identity("tags", 10)
    with pytest.raises(ValueError, match="weighted"):
        fc.crossed_column(["workclass", fc.weighted_categorical_column(ident, "w")], 128)
    with pytest.raises(ValueError):
        fc.crossed_column(["k%d" % i for i in range(9)], 128)

    c = fc.crossed_column(["workclass", "education"], 128)
    assert c.name == "education_X_workclass" and c.num_buckets == 128 and c.hash_key == KEY
    assert c.keys == ("workclass", "education") and c.is_categorical and not c.range_checked and c.weight_key is None
    assert fc.embedding_column(c, 8).name == "education_X_workclass_embedding"
    assert fc.indicator_column(c).name == "education_X_workclass_indicator" and fc.indicator_column(c).dimension == 128
    # a nested cross is flattened to its leaf keys, in order; a categorical column is a leaf and gives its name
    n = fc.crossed_column([c, ident, "age"], 7, hash_key=5)
    assert n.keys == ("workclass", "education", ident, "age") and n.name == "age_X_education_X_tags_X_workclass" and n.hash_key == 5
    # the name is sorted, the hashing order is the order given
    r = fc.crossed_column(["education", "workclass"], 128)
    assert r.name == c.name and r.keys != c.keys
    assert S.cross_id([3, 7], 128) != S.cross_id([7, 3], 128)


def test_crossed_column_refuses_float_features(built_lib):
    import torch
    from dir_amd import feature_column as fc
    c = fc.crossed_column(["a", "b"], 16)
    with pytest.raises(TypeError):
        c.ids({"a": torch.zeros(3), "b": torch.zeros(3, dtype=torch.int64)}, "cpu")


def test_crossed_linear_column_checkpoint_name(built_lib):
    from dir_amd import feature_column as fc
    from dir_amd.checkpoint import tf_variable_map
    from dir_amd.deepfm import DeepFM
    crossed = fc.crossed_column(["workclass", "education"], 128)
    embs = [fc.embedding_column(fc.categorical_column_with_identity("C%d" % i, 30), 4) for i in range(3)]
    model = DeepFM(linear_feature_columns=[crossed], dnn_feature_columns=embs, dnn_hidden_units=[8, 4], fm_embedding_size=4)
    m = tf_variable_map(model)
    assert "linear/linear_model/education_X_workclass/weights" in m
    assert m["linear/linear_model/education_X_workclass/weights"][0].shape[0] == 128


def test_serving_export_parses_the_leaf_keys_of_a_crossed_column(built_lib, tmp_path):
    import json
    import os
    from dir_amd import feature_column as fc
    from dir_amd.checkpoint import export_serving
    from dir_amd.deepfm import DeepFM
    tags = fc.categorical_column_with_identity("tags", 10)
    crossed = fc.crossed_column(["workclass", "education", tags], 128)
    embs = [fc.embedding_column(fc.categorical_column_with_identity("C%d" % i, 30), 4) for i in range(2)]
    model = DeepFM(linear_feature_columns=[crossed], dnn_feature_columns=embs, dnn_hidden_units=[8], fm_embedding_size=4)
    exp = export_serving(model, str(tmp_path / "export"))
    spec = json.load(open(os.path.join(exp, "serving_signature.json")))["feature_spec"]
    assert sorted(spec) == ["C0", "C1", "education", "tags", "workclass"]
    assert spec["workclass"] == spec["education"] == {"kind": "VarLenFeature", "dtype": "string"}
    assert spec["tags"] == {"kind": "VarLenFeature", "dtype": "int64"}


def test_standin_product_order():
    """Row 0: key a holds [10, 11], key b holds [20, 21, 22] -> (10,20) (10,21) (10,22) (11,20) (11,21) (11,22): the last key fastest.
    Row 1: b is empty -> no entries.  Row 2: one entry each."""
    a = ([10, 11, 12, 13], [0, 2, 3, 4])
    b = ([20, 21, 22, 23], [0, 3, 3, 4])
    ids, offs = S.cross_ragged([a, b], 1 << 62)
    assert offs.tolist() == [0, 6, 6, 7]
    want = [(10, 20), (10, 21), (10, 22), (11, 20), (11, 21), (11, 22), (13, 23)]
    assert ids.tolist() == [S.cross_id(p, 1 << 62) for p in want]
    # a one-hot key counts as length 1
    ids2, offs2 = S.cross_ragged([[5, 6, 7], b], 1000)
    assert offs2.tolist() == [0, 3, 3, 4] and ids2.tolist() == [S.cross_id(p, 1000) for p in [(5, 20), (5, 21), (5, 22), (7, 23)]]
    assert S.cross_onehot([[3], [7]], 128).tolist() == [41]
