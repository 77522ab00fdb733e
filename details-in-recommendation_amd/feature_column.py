"""feature_column.py -- light shims of the tf.feature_column constructors the reference uses.

They carry only what the hot path needs (name, key, num_buckets, dimension, combiner, boundaries,
vocabulary) and turn a raw feature into int64 ids:
  identity  : id in [0, num_buckets) else default_value          models/LFM/Mixture_1/train.py:34-37
  hash      : FarmHash Fingerprint64(str(x)) mod buckets         models/DeepCrossNetwork/train.py:85-86
  vocabulary: index in the list, OOV -> -1 (dropped by the bag)  models/DeepCrossNetwork/train.py:63-82
  bucketized: number of boundaries <= x                          models/DeepFM/deepFM.py:95 (docstring)
  crossed   : FingerprintCat64 chain over the keys mod buckets   models/ESMM/train.py:94
and the dense wrappers: embedding_column, indicator_column, shared_embedding_columns (several id columns on ONE table,
models/DeepFM/test02.py:30: the models hold one parameter per table, see table_slots).
Column names follow [TF-upstream] naming (`<key>_embedding`, `<key>_indicator`, `<key>_bucketized`, `<a>_X_<b>`) because
DCN's input_layer concatenates columns sorted by name (DeepCrossNetwork.py:126).
"""
import numbers
from collections import namedtuple

import torch

from . import ops

# A variable-length (multi-hot) feature: CSR over the batch, the dense stand-in for the SparseTensor a
# TF categorical column receives.  values [nnz] (ids or raw keys), offsets [B+1] int64, weights [nnz]|None.
Ragged = namedtuple("Ragged", ["values", "offsets", "weights"], defaults=[None])


class _Column:
    is_dense = False
    is_categorical = False


class NumericColumn(_Column):
    is_dense = True

    def __init__(self, key, shape=(1,)):
        self.key = key
        self.name = key
        self.shape = tuple(shape)
        self.dimension = 1
        for s in self.shape:
            self.dimension *= int(s)


class _Categorical(_Column):
    is_categorical = True
    weight_key = None

    def ids(self, features, device):
        """-> one-hot LongTensor [B]  or  multi-hot (values [nnz], offsets [B+1], weights|None)."""
        raw = features[self.key]
        if isinstance(raw, Ragged):
            vals = self._to_ids(raw.values, device)
            w = raw.weights
            return vals, raw.offsets.to(device=device, dtype=torch.int64), (w.to(device) if w is not None else None)
        t = self._to_ids(raw, device)
        return t.reshape(-1)

    def _to_ids(self, raw, device):
        raise NotImplementedError


class IdentityCategoricalColumn(_Categorical):
    def __init__(self, key, num_buckets, default_value=None):
        if num_buckets is None or num_buckets < 1:
            raise ValueError("num_buckets {} < 1, column_name {}".format(num_buckets, key))
        if default_value is not None and not (0 <= default_value < num_buckets):
            raise ValueError("default_value {} not in range [0, {}), column_name {}".format(default_value, num_buckets, key))
        self.key = key
        self.name = key
        self.num_buckets = int(num_buckets)
        self.default_value = default_value

    @property
    def range_checked(self):
        """Without a default_value TensorFlow asserts 0 <= id < num_buckets (see _input.check_id_range)."""
        return self.default_value is None

    def _to_ids(self, raw, device):
        t = raw.to(device=device, dtype=torch.int64)
        if self.default_value is not None:
            bad = (t < 0) | (t >= self.num_buckets)
            t = torch.where(bad, torch.full_like(t, int(self.default_value)), t)
        return t


class HashedCategoricalColumn(_Categorical):
    def __init__(self, key, hash_bucket_size):
        if hash_bucket_size is None or hash_bucket_size < 1:
            raise ValueError("hash_bucket_size must be at least 1")
        self.key = key
        self.name = key
        self.num_buckets = int(hash_bucket_size)

    def _to_ids(self, raw, device):
        if isinstance(raw, torch.Tensor):  # integer keys: hashed on the device as decimal text
            return ops.hash_bucket_ints(raw.to(device=device, dtype=torch.int64).reshape(-1), self.num_buckets)
        return ops.hash_bucket_strings(list(raw), self.num_buckets).to(device)


class VocabularyListCategoricalColumn(_Categorical):
    def __init__(self, key, vocabulary_list, default_value=-1):
        self.key = key
        self.name = key
        self.vocabulary = {v: i for i, v in enumerate(vocabulary_list)}
        self.num_buckets = len(self.vocabulary)
        self.default_value = default_value

    def _to_ids(self, raw, device):
        if isinstance(raw, torch.Tensor):
            raw = raw.reshape(-1).tolist()
        return torch.tensor([self.vocabulary.get(v, self.default_value) for v in raw], dtype=torch.int64, device=device)


class BucketizedColumn(_Categorical):
    def __init__(self, source_column, boundaries):
        self.key = source_column.key
        self.name = source_column.key + "_bucketized"
        self.boundaries = [float(b) for b in boundaries]
        if sorted(self.boundaries) != self.boundaries:
            raise ValueError("boundaries must be sorted")
        self.num_buckets = len(self.boundaries) + 1
        self._bd = None

    def _to_ids(self, raw, device):
        if self._bd is None or self._bd.device != torch.device(device):
            self._bd = torch.tensor(self.boundaries, dtype=torch.float32, device=device)
        return ops.bucketize(raw.to(device=device, dtype=torch.float32).reshape(-1), self._bd)


class WeightedCategoricalColumn(_Categorical):
    range_checked = property(lambda self: getattr(self.categorical_column, "range_checked", False))

    """weighted_categorical_column (dataset/SequenceTensorFlowDataset/test4.py:53): ids from the wrapped
    column, per-entry weights from features[weight_feature_key] (same ragged layout)."""

    def __init__(self, categorical_column, weight_feature_key):
        self.categorical_column = categorical_column
        self.key = categorical_column.key
        self.weight_key = weight_feature_key
        self.name = "%s_weighted_by_%s" % (categorical_column.name, weight_feature_key)
        self.num_buckets = categorical_column.num_buckets

    def ids(self, features, device):
        got = self.categorical_column.ids(features, device)
        if not isinstance(got, tuple):
            raise ValueError("weighted_categorical_column needs a Ragged (multi-hot) feature")
        vals, offs, _ = got
        w = features[self.weight_key]
        if isinstance(w, Ragged):
            w = w.values
        return vals, offs, w.to(device=device, dtype=torch.float32).reshape(-1)


class CrossedColumn(_Categorical):
    """crossed_column (models/ESMM/train.py:94).  [TF-upstream] _CrossedColumn / SparseCross with hashed output, stated and not verified
    (DESIGN.md section 2): every leaf key gives 64 bits per entry -- an integer feature as it is, a string feature's Fingerprint64, a
    categorical column's ids as column.ids() returns them --, chained through FingerprintCat64 from hash_key IN THE ORDER GIVEN, modulo
    hash_bucket_size.  Nothing is dropped (-1 and "" are crossed like any value); the ids are in range by construction; no weights."""
    is_crossed = True
    range_checked = False

    def __init__(self, keys, hash_bucket_size, hash_key=None):
        if hash_bucket_size is None or hash_bucket_size < 1:
            raise ValueError("hash_bucket_size must be at least 1. hash_bucket_size: {}".format(hash_bucket_size))
        if not keys or len(keys) < 2:
            raise ValueError("keys must be a list with length > 1. Given: {}".format(keys))
        leaves = []
        for k in keys:
            if isinstance(k, CrossedColumn):
                leaves += k.keys                      # a nested cross is its leaf keys, in order
            elif isinstance(k, HashedCategoricalColumn):
                raise ValueError("categorical_column_with_hash_bucket is not supported for crossing. Hashing before crossing will increase "
                                 "probability of collision. Instead, use the feature name as a string. Given: {}".format(k.name))
            elif isinstance(k, WeightedCategoricalColumn):
                raise ValueError("a weighted_categorical_column cannot be crossed (a crossed column carries no weights). Given: {}".format(k.name))
            elif isinstance(k, (str, _Categorical)):
                leaves.append(k)
            else:
                raise ValueError("Unsupported key type. All keys must be either string, or categorical column. Given: {}".format(k))
        if len(leaves) > ops.CROSS_MAX_KEYS:
            raise ValueError("a crossed column takes at most %d leaf keys, got %d" % (ops.CROSS_MAX_KEYS, len(leaves)))
        self.keys = tuple(leaves)
        self.num_buckets = int(hash_bucket_size)
        self.hash_key = ops.CROSS_HASH_KEY if hash_key is None else int(hash_key)
        self.name = "_X_".join(sorted(k if isinstance(k, str) else k.name for k in leaves))
        self.key = self.name

    def ids(self, features, device):
        return cross_columns([self], features, device)[0]


def _cross_contribution(leaf, features, device):
    """A leaf key's 64 bits per entry: -> int64 [B], or (values [nnz], offsets [B+1]) for a Ragged feature."""
    if not isinstance(leaf, str):
        got = leaf.ids(features, device)
        return (got[0], got[1]) if isinstance(got, tuple) else got

    def bits(raw):
        if isinstance(raw, torch.Tensor):
            if raw.dtype.is_floating_point or raw.dtype == torch.bool:
                raise TypeError("crossed_column key %r: a %s feature cannot be crossed (integer or string keys only)" % (leaf, raw.dtype))
            return raw.to(device=device, dtype=torch.int64).reshape(-1)
        raw = list(raw)
        if raw and all(isinstance(v, numbers.Integral) for v in raw):
            return torch.tensor([int(v) for v in raw], dtype=torch.int64, device=device)
        if any(isinstance(v, numbers.Number) for v in raw):
            raise TypeError("crossed_column key %r: a float feature cannot be crossed (integer or string keys only)" % leaf)
        return ops.fingerprint64_strings(raw).to(device)      # one host call for the batch, one upload

    raw = features[leaf]
    if isinstance(raw, Ragged):
        return bits(raw.values), raw.offsets.to(device=device, dtype=torch.int64)
    return bits(raw)


def cross_columns(columns, features, device):
    """The ids of several crossed columns over one features dict: a leaf key they share is turned into its contribution once, and ALL the
    one-hot crosses are formed by one launch into one field-major [NX, B] matrix whose rows are handed out as views (what
    _input.collect_ids wants: a linear model over crosses reads that matrix in place).  -> a list as column.ids() would give."""
    srcs, index = [], {}
    plans = []
    for c in columns:
        ks = []
        for leaf in c.keys:
            ident = leaf if isinstance(leaf, str) else id(leaf)
            if ident not in index:
                index[ident] = len(srcs)
                srcs.append(_cross_contribution(leaf, features, device))
            ks.append(index[ident])
        plans.append(ks)
    out = [None] * len(columns)
    dense = [i for i, ks in enumerate(plans) if not any(isinstance(srcs[k], tuple) for k in ks)]
    if dense:
        used = list(dict.fromkeys(k for i in dense for k in plans[i]))
        local = {k: j for j, k in enumerate(used)}
        mat = ops.cross_hash([srcs[k] for k in used],
                             [([local[k] for k in plans[i]], columns[i].num_buckets, columns[i].hash_key) for i in dense])
        for j, i in enumerate(dense):
            out[i] = mat[j]
    for i, ks in enumerate(plans):
        if out[i] is None:
            vals, offs = ops.cross_hash_ragged([srcs[k] for k in ks], columns[i].num_buckets, columns[i].hash_key)
            out[i] = (vals, offs, None)
    return out


class EmbeddingColumn(_Column):
    is_dense = True

    def __init__(self, categorical_column, dimension, combiner="mean", max_norm=None):
        if dimension is None or dimension < 1:
            raise ValueError("Invalid dimension {}.".format(dimension))
        if combiner not in ("mean", "sqrtn", "sum"):
            raise ValueError("combiner must be one of mean, sqrtn, sum")
        self.categorical_column = categorical_column
        self.dimension = int(dimension)
        self.combiner = combiner
        self.max_norm = max_norm          # [TF-upstream] embedding_column(max_norm=): l2-clip every looked-up row
        self.name = categorical_column.name + "_embedding"
        self.num_buckets = categorical_column.num_buckets


class SharedEmbeddingColumn(EmbeddingColumn):
    """One of the columns shared_embedding_columns returns (models/DeepFM/test02.py:30): an embedding column whose table belongs to a
    collection.  Columns of one model with the same shared_embedding_collection_name read and train ONE [num_buckets, dimension] table."""

    def __init__(self, categorical_column, dimension, combiner, max_norm, shared_embedding_collection_name):
        super().__init__(categorical_column, dimension, combiner, max_norm)
        self.name = categorical_column.name + "_shared_embedding"
        self.shared_embedding_collection_name = shared_embedding_collection_name


def table_key(column):
    """What names a dense column's embedding table inside one model: the collection of a shared column, the column itself otherwise."""
    shared = getattr(column, "shared_embedding_collection_name", None)
    return ("shared", shared) if shared is not None else ("column", id(column))


def var_scope_name(column):
    """The variable scope of a column's embedding table ([TF-upstream] column._var_scope_name, test02.py:84): the collection name of a
    shared column, the column's own name otherwise."""
    return getattr(column, "shared_embedding_collection_name", None) or column.name


def table_slots(columns):
    """columns -> (slot_table, firsts): slot_table[i] = the index of column i's table among the distinct tables (in order of first
    appearance), firsts[t] = the first column of table t.  One collection name must mean one (num_buckets, dimension) here."""
    index, slot_table, firsts = {}, [], []
    for c in columns:
        k = table_key(c)
        if k not in index:
            index[k] = len(firsts)
            firsts.append(c)
        first = firsts[index[k]]
        if (first.num_buckets, first.dimension) != (c.num_buckets, c.dimension):
            raise ValueError("shared_embedding_collection_name %r names tables of different shapes: %s is (%d, %d), %s is (%d, %d)" % (
                c.shared_embedding_collection_name, first.name, first.num_buckets, first.dimension, c.name, c.num_buckets, c.dimension))
        slot_table.append(index[k])
    return slot_table, firsts


def first_shared(columns):
    """-> the first column among `columns` that shares its table with another one of them, or None."""
    cols = [c for c in columns if isinstance(c, EmbeddingColumn)]
    slot_table, _ = table_slots(cols)
    for i, t in enumerate(slot_table):
        if slot_table.count(t) > 1:
            return cols[i]
    return None


class IndicatorColumn(_Column):
    is_dense = True

    def __init__(self, categorical_column):
        self.categorical_column = categorical_column
        self.dimension = categorical_column.num_buckets
        self.name = categorical_column.name + "_indicator"


def numeric_column(key, shape=(1,)):
    return NumericColumn(key, shape)


def categorical_column_with_identity(key, num_buckets, default_value=None):
    return IdentityCategoricalColumn(key, num_buckets, default_value)


def categorical_column_with_hash_bucket(key, hash_bucket_size, dtype=None):
    return HashedCategoricalColumn(key, hash_bucket_size)


def categorical_column_with_vocabulary_list(key, vocabulary_list, dtype=None, default_value=-1):
    return VocabularyListCategoricalColumn(key, vocabulary_list, default_value)


def bucketized_column(source_column, boundaries):
    return BucketizedColumn(source_column, boundaries)


def weighted_categorical_column(categorical_column, weight_feature_key):
    return WeightedCategoricalColumn(categorical_column, weight_feature_key)


def crossed_column(keys, hash_bucket_size, hash_key=None):
    return CrossedColumn(keys, hash_bucket_size, hash_key)


def embedding_column(categorical_column, dimension, combiner="mean", max_norm=None):
    return EmbeddingColumn(categorical_column, dimension, combiner, max_norm)


def shared_embedding_columns(categorical_columns, dimension, combiner="mean", shared_embedding_collection_name=None, max_norm=None):
    """[TF-upstream] shared_embedding_columns (r1.10-r1.13; models/DeepFM/test02.py:30), stated and not verified like the rest of this
    file: one dense column per categorical column IN THE ORDER GIVEN, named <categorical.name>_shared_embedding, all reading one table.
    The default collection name is the categorical columns' names, sorted, joined by "_", plus "_shared_embedding"."""
    categorical_columns = list(categorical_columns or [])
    if not categorical_columns:
        raise ValueError("categorical_columns must be a non-empty list.")
    if dimension is None or dimension < 1:
        raise ValueError("Invalid dimension {}.".format(dimension))
    buckets = categorical_columns[0].num_buckets
    for c in categorical_columns[1:]:
        if c.num_buckets != buckets:
            raise ValueError("To use shared_embedding_column, all categorical_columns must have the same number of buckets. "
                             "Given column: {} with buckets: {} does not match column: {} with buckets: {}".format(
                                 categorical_columns[0].name, buckets, c.name, c.num_buckets))
    if not shared_embedding_collection_name:
        shared_embedding_collection_name = "_".join(sorted(c.name for c in categorical_columns)) + "_shared_embedding"
    return [SharedEmbeddingColumn(c, dimension, combiner, max_norm, shared_embedding_collection_name) for c in categorical_columns]


def indicator_column(categorical_column):
    return IndicatorColumn(categorical_column)
