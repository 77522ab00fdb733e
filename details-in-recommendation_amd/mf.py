"""mf.py -- the matrix-factorisation family of the reference on the fused HIP score kernels (csrc/mf.hip).

  BiasedMF   models/LFM/Mixture_1/MF_model.py (BaseMFModel): R[u, i] = b0 + bu[u] + bi[i] + P[u] . Q[i], mse or (weighted) log loss,
             reg_pen * l2_loss of the looked-up rows.  _logit_fn :164-194, the label lines :124-145 and _get_loss :196-215 are restated here;
             models/LFM/Biased LFM/inference.py:48-50 is the same regulariser.
  Svd        models/LFM/Mixture_2/model.py:74-90: no biases, mean sigmoid cross-entropy; BiasedMF with intercepts=False.
  BPR        paper-derived (Rendle et al., "BPR: Bayesian Personalized Ranking from Implicit Feedback", UAI 2009): the reference holds no
             model text for it, only the pair-wise sampler models/BPR/bpr_sampler.py:102-111, whose distribution ops.neg_sample reproduces
             on the device without its rejection loop.

On a CUDA (ROCm) device the scores are ONE launch of dir_mf_score_f32 over ids = [user | items] and the backward one launch of
dir_mf_score_backward_f32, which also produces the regulariser's gradient (its l2 terms): create_loss adds the regulariser's VALUE only
there.  device="cpu" runs a torch formulation of the same formulas (for host tests; there the regulariser carries its own graph).
Not built: BiasedSvd's trainable alpha, the Estimator loop, the CSV / vocabulary-file pipeline of bpr_sampler.py (ids arrive as indices).
"""
import math

import torch
from torch import nn

from . import autograd as ag
from . import ops
from .feature_column import EmbeddingColumn


def _one_column(c, what):
    """The reference hands tf.feature_column.input_layer ONE column per call (MF_model.py:168-173); a one-element list is the same."""
    if isinstance(c, (list, tuple)):
        if len(c) != 1:
            raise ValueError("%s: one embedding column, got %d" % (what, len(c)))
        c = c[0]
    if not isinstance(c, EmbeddingColumn):
        raise ValueError("Items of feature_columns must be a _DenseColumn. Given: {}".format(c))
    return c


def _table(rows, dim):
    s = 1.0 / math.sqrt(dim)          # [TF-upstream] embedding_column default initializer
    return nn.Parameter(nn.init.trunc_normal_(torch.empty(rows, dim), std=s, a=-2 * s, b=2 * s))


def _l2_loss(*ts):
    """sum of tf.nn.l2_loss(t) = sum(t ** 2) / 2"""
    return sum((t * t).sum() for t in ts) / 2.0


class _MFBase(nn.Module):
    """The four variables and the two score paths.  Subclasses set _SCOPE (the reference's variable scope)."""
    _SCOPE = "inputs"

    def _init_tables(self, num_users, num_items, dim, intercepts, global_bias):
        self.num_users, self.num_items, self.dim, self.intercepts = int(num_users), int(num_items), int(dim), bool(intercepts)
        self.user_emb, self.item_emb = _table(self.num_users, self.dim), _table(self.num_items, self.dim)
        if self.intercepts:
            self.user_bias, self.item_bias = _table(self.num_users, 1), _table(self.num_items, 1)
        else:
            self.register_parameter("user_bias", None)
            self.register_parameter("item_bias", None)
        if global_bias and self.intercepts:
            self.global_bias = nn.Parameter(torch.zeros(()))             # MF_model.py:174-175: shape [], zeros
        else:
            self.register_parameter("global_bias", None)
        self._sinks = (None, None)                                       # (row sink, bias sink) of the fused sparse optimisers
        self._sink_C = None
        self._register_state_dict_hook(self._tf_names_out)
        self._register_load_state_dict_pre_hook(self._tf_names_in)

    # ---- state_dict under the reference's variable names ---------------------------------------------------------------------------
    def tf_names(self):
        """{attribute: the reference graph's variable name}.  [TF-upstream] every input_layer call opens a fresh `input_layer` scope,
        uniquified in call order (MF_model.py:168-173: user_emb, item_emb, user_bias, item_bias)."""
        s, u, i = self._SCOPE, self._user_col_name, self._item_col_name
        m = {"user_emb": "%s/input_layer/%s/embedding_weights" % (s, u), "item_emb": "%s/input_layer_1/%s/embedding_weights" % (s, i)}
        if self.intercepts:
            m["user_bias"] = "%s/input_layer_2/%s/embedding_weights" % (s, self._user_bias_col_name)
            m["item_bias"] = "%s/input_layer_3/%s/embedding_weights" % (s, self._item_bias_col_name)
        if self.global_bias is not None:
            m["global_bias"] = "%s/global_bias" % s
        return m

    @staticmethod
    def _tf_names_out(module, state, prefix, local_metadata):
        for attr, name in module.tf_names().items():
            if prefix + attr in state:
                state[prefix + name] = state.pop(prefix + attr)
        return state

    def _tf_names_in(self, state, prefix, *args):
        for attr, name in self.tf_names().items():
            if prefix + name in state:
                state[prefix + attr] = state.pop(prefix + name)

    # ---- scores ---------------------------------------------------------------------------------------------------------------------
    def _l2(self):
        return 0.0

    def _rows(self, ids):
        """The looked-up rows of ids [B, 1 + C] (torch index ops): (P[u] [B, K], Q[i] [B, C, K], bu[u] [B, 1] | None, bi[i] [B, C] | None)."""
        u, it = ids[:, 0], ids[:, 1:]
        pu, qi = self.user_emb[u], self.item_emb[it]
        if not self.intercepts:
            return pu, qi, None, None
        return pu, qi, self.user_bias[u], self.item_bias[it].squeeze(-1)

    def _scores(self, ids):
        """ids int64 [B, 1 + C] -> scores [B, C]: the HIP kernel on a CUDA device, the torch formulation on the CPU."""
        if ids.device != self.user_emb.device:
            ids = ids.to(self.user_emb.device)
        if not self.user_emb.is_cuda:
            pu, qi, bu, bi = self._rows(ids)
            s = (pu.unsqueeze(1) * qi).sum(-1)
            if bu is not None:
                b = bu + bi
                s = s + (b + self.global_bias if self.global_bias is not None else b)       # (bu + bi) + b0: MF_model.py:184
            return s
        if torch.is_grad_enabled() and self.user_emb.requires_grad:
            rs, bs = self._sinks
            if rs is not None and ids.shape[1] - 1 != self._sink_C:
                raise ValueError("the fused sparse optimiser was attached for C = %d item slots, this batch has %d" % (self._sink_C, ids.shape[1] - 1))
            if rs is not None and self._mf_ts[0].tables[0].data_ptr() != self.user_emb.data_ptr():
                ops.refuse_rebuild_under_sink(*self._mf_ts)      # the tables moved after the optimiser was attached: it holds the old storage
            return ag.mf_score(self.user_emb, self.item_emb, ids, self.user_bias, self.item_bias, self.global_bias, l2=self._l2(),
                               row_sink=rs, bias_sink=bs)
        d = lambda p: p.data if p is not None else None      # noqa: E731
        return ops.mf_score(self.user_emb.data, self.item_emb.data, ids, d(self.user_bias), d(self.item_bias), d(self.global_bias))

    def _reg(self, ids, coef):
        """coef * (l2_loss of the looked-up rows and biases), per occurrence (MF_model.py:200-206).  On the HIP path the value only: its
        gradient is the l2 terms of the score's backward."""
        if not coef:
            return 0.0
        if self.user_emb.is_cuda:
            with torch.no_grad():
                return coef * _l2_loss(*[t for t in self._rows(ids) if t is not None])
        return coef * _l2_loss(*[t for t in self._rows(ids) if t is not None])

    # ---- fused sparse optimisers ----------------------------------------------------------------------------------------------------
    def _fused(self, C, make):
        """One optimiser over TableSet([P] + [Q] * C) -- a sharing set: a row's gradients from all its slots are summed once and applied
        once -- and, where the optimiser takes K = 1, a second one over TableSet([bu] + [bi] * C).  make(ts) -> an optimiser or None."""
        if not self.user_emb.is_cuda:
            raise RuntimeError("the fused sparse optimisers live on a CUDA (ROCm) device: move the model first")
        rows =ops.TableSet([self.user_emb.data] + [self.item_emb.data] * C)
        rows.owners = [self.user_emb, self.item_emb]
        opt = make(rows)
        if opt is None:
            raise ValueError("the fused optimiser does not cover K = %d with C = %d item slots" % (self.dim, C))
        bias_opt = None
        self._mf_ts = (rows,)
        if self.intercepts:
            bias = ops.TableSet([self.user_bias.data] + [self.item_bias.data] * C)
            bias.owners = [self.user_bias, self.item_bias]
            bias_opt = make(bias)
            if bias_opt is not None:
                self._mf_ts = (rows, bias)
        rows.grad_sink = opt.step
        if bias_opt is not None:
            bias_opt.ts.grad_sink = bias_opt.step
        self._sinks, self._sink_C = (opt.step, bias_opt.step if bias_opt is not None else None), C
        self._sparse_opts = (opt, bias_opt)
        return opt, bias_opt

    def _fused_adagrad(self, C, lr, initial_accumulator_value):
        return self._fused(C, lambda ts: ops.SparseAdagrad(ts, lr, initial_accumulator_value=initial_accumulator_value, method="sorted"))

    def _fused_adam(self, C, beta1, beta2, eps, clip_norm):
        return self._fused(C, lambda ts: ops.SparseAdam(ts, beta1, beta2, eps, clip_norm, shared=True) if ops.SparseAdam.covers(ts) else None)


class BiasedMF(_MFBase):
    """BaseMFModel (models/LFM/Mixture_1/MF_model.py:54-66), with its constructor keywords.  embedding_cols = [user, item]
    fc.embedding_column(fc.categorical_column_with_identity(key, n), K); bias_cols = the same two categoricals as embedding_column(..., 1)
    (not read with intercepts=False).  model_dir, learning_rate, optimizer and config are kept for the caller's training loop.

    forward({user key, item key}) -> logits [B, 1]; predict(features) -> the reference's prediction dict; create_loss(features, logits,
    labels) -> the reference's cost.  fused_sparse_adagrad / fused_sparse_adam attach the HIP sparse steps (one item slot)."""

    def __init__(self, model_dir=None, embedding_cols=None, bias_cols=None, reg_pen=None, learning_rate=None, is_implicit=False, loss='mse',
                 intercepts=True, optimizer='Adam', weights=None, weights_coef=0, config=None):
        super().__init__()
        if loss not in ['mse', 'cross entropy']:
            raise ValueError("use 'mse' or 'cross entropy' loss")
        if optimizer not in ['Adam', 'Ftrl', None]:
            raise ValueError("use 'Adam' or 'Ftrl' optimizer or None")
        if weights not in ['log_weight', 'normal_weight', None]:
            raise ValueError("use 'log_weight' or 'normal_weight' weights or None")
        ucol, icol = _one_column(embedding_cols[0], "embedding_cols[0]"), _one_column(embedding_cols[1], "embedding_cols[1]")
        if ucol.dimension != icol.dimension:
            raise ValueError("the user and item embedding columns must share one dimension, got %d and %d" % (ucol.dimension, icol.dimension))
        self.user_key, self.item_key = ucol.categorical_column.key, icol.categorical_column.key
        self._user_col_name, self._item_col_name = ucol.name, icol.name
        self._user_bias_col_name, self._item_bias_col_name = ucol.name, icol.name
        if intercepts:
            ub, ib = _one_column(bias_cols[0], "bias_cols[0]"), _one_column(bias_cols[1], "bias_cols[1]")
            if ub.dimension != 1 or ib.dimension != 1 or ub.num_buckets != ucol.num_buckets or ib.num_buckets != icol.num_buckets:
                raise ValueError("bias_cols must be embedding columns of dimension 1 over the same categorical columns")
            self._user_bias_col_name, self._item_bias_col_name = ub.name, ib.name
        self.model_dir, self.config = model_dir, config
        self.reg_pen, self.learning_rate = reg_pen, learning_rate
        self.is_implicit, self.loss, self.optimizer = is_implicit, loss, optimizer
        self.weights, self.weights_coef = weights, weights_coef
        self._init_tables(ucol.num_buckets, icol.num_buckets, ucol.dimension, intercepts, global_bias=True)

    def _l2(self):
        return float(self.reg_pen or 0.0)

    def ids_of(self, features):
        dev = self.user_emb.device
        u = features[self.user_key].to(device=dev, dtype=torch.int64).reshape(-1)
        i = features[self.item_key].to(device=dev, dtype=torch.int64).reshape(-1)
        if u.numel() != i.numel():
            raise ValueError("features %r and %r disagree on the batch size" % (self.user_key, self.item_key))
        return torch.stack([u, i], dim=1)

    def forward(self, features):
        return self._scores(self.ids_of(features))

    def _preds(self, logits):
        return torch.sigmoid(logits) if self.loss == "cross entropy" else logits

    @torch.no_grad()
    def predict(self, features):
        """MF_model.py:106-118."""
        logits = self.forward(features)
        preds = self._preds(logits)
        if self.loss != "cross entropy":
            return {"scores": preds}
        probabilities = torch.softmax(torch.cat((torch.zeros_like(logits), logits), dim=-1), dim=-1)
        return {"probabilities": probabilities, "logistic": preds, "class_ids": torch.argmax(probabilities, dim=-1).unsqueeze(-1)}

    def label_weights(self, labels, label_threshold=4.0):
        """MF_model.py:124-145 restated -> (labels [B, 1], weights [B] or 1.0).  label_threshold None: the labels are taken as they are."""
        labels = labels.to(device=self.user_emb.device, dtype=torch.float32).reshape(-1)
        if label_threshold is not None:
            labels = (labels >= float(label_threshold)).to(torch.float32)
        term = 0.0
        if self.is_implicit:
            labels = labels.clamp(0, 1)
            if self.weights == "log_weight":
                term = torch.log1p(labels)
            elif self.weights == "normal_weight":
                term = labels
        weights = 1.0 + self.weights_coef * term
        return labels.unsqueeze(-1), weights

    def data_loss(self, preds, labels, weights):
        """tf.losses.log_loss (epsilon 1e-7) / mean_squared_error with their default reduction: the weighted sum over the number of
        non-zero weights (MF_model.py:209-212).  weights: a scalar or [B], broadcast over labels [B, 1] as [B, 1]."""
        if self.loss == "cross entropy":
            eps = 1e-7
            per = -labels * torch.log(preds + eps) - (1.0 - labels) * torch.log(1.0 - preds + eps)
        else:
            per = (preds - labels) ** 2
        w = torch.as_tensor(weights, dtype=per.dtype, device=per.device)
        w = (w.reshape(-1, 1) if w.dim() else w).expand_as(per)
        nz = (w != 0).sum().to(per.dtype)
        total = (per * w).sum()
        return torch.where(nz > 0, total / nz.clamp_min(1.0), torch.zeros_like(total))

    def create_loss(self, features, logits, labels, label_threshold=4.0):
        """cost = loss + reg_pen * (l2_loss of the looked-up rows and biases) (MF_model.py:196-215)."""
        y, w = self.label_weights(labels, label_threshold)
        return self.data_loss(self._preds(logits), y, w) + self._reg(self.ids_of(features), self._l2())

    def fused_sparse_adagrad(self, lr, initial_accumulator_value=0.1):
        """Attach ops.SparseAdagrad (sorted method) to [P, Q] and to [bu, bi] (the sorted Adagrad step takes K = 1): backward() then updates
        the four variables in place and they get no .grad; global_bias keeps its dense .grad.  -> (row optimiser, bias optimiser | None)."""
        return self._fused_adagrad(1, lr, initial_accumulator_value)

    def fused_sparse_adam(self, beta1=0.9, beta2=0.999, eps=1e-8, clip_norm=0.0):
        """Attach ops.SparseAdam(shared=True) to [P, Q] where SparseAdam.covers it.  The Adam step needs K % 4 == 0, so the biases (K = 1)
        keep their sparse .grad for a torch optimiser.  Set .lr_t on the returned optimiser before every backward."""
        return self._fused_adam(1, beta1, beta2, eps, clip_norm)


class Svd(BiasedMF):
    """models/LFM/Mixture_2/model.py (Svd): no biases, mean sigmoid cross-entropy on the labels as given, l2_pen * l2_loss of the looked-up
    rows (:74-90), with its keywords: user_emb / item_emb are the two embedding columns."""
    _SCOPE = "input_from_feature_columns"

    def __init__(self, user_emb=None, item_emb=None, l2_pen=None, learning_rate=None, model_dir=None, config=None):
        super().__init__(model_dir=model_dir, embedding_cols=[user_emb, item_emb], bias_cols=None, reg_pen=l2_pen, learning_rate=learning_rate,
                         loss='cross entropy', intercepts=False, optimizer='Adam', config=config)
        self.l2_pen = l2_pen

    def create_loss(self, features, logits, labels, label_threshold=None):
        y, _ = self.label_weights(labels, label_threshold)
        return nn.functional.binary_cross_entropy_with_logits(logits, y) + self._reg(self.ids_of(features), self._l2())


class BPR(_MFBase):
    """Bayesian Personalized Ranking -- paper-derived (Rendle et al., UAI 2009): x_ui = P[u] . Q[i] + bu[u] + bi[i], the loss
    mean(-log sigmoid(x_ui - x_uj)) over sampled (u, i, j) + reg_pen * l2_loss of the looked-up rows.  The reference has the sampler only
    (models/BPR/bpr_sampler.py:102-111): sample() draws j on the device from the items u has not interacted with.

    user_items: an ops.UserItems (needed by sample()).  sampler_rng: an ops.DropoutState, advanced once per sample(), so a captured step
    replays with fresh negatives; it is not part of state_dict()."""

    def __init__(self, num_users, num_items, dimension, reg_pen=0.0, n_neg=1, user_items=None, intercepts=True, seed=None):
        super().__init__()
        if int(n_neg) < 1:
            raise ValueError("n_neg must be at least 1")
        self._user_col_name = self._user_bias_col_name = "user_embedding"
        self._item_col_name = self._item_bias_col_name = "item_embedding"
        self.reg_pen, self.n_neg, self.user_items, self._seed = float(reg_pen), int(n_neg), user_items, seed
        self.sampler_rng = None
        self._last_ids = None
        self._init_tables(num_users, num_items, dimension, intercepts, global_bias=False)      # (a global bias cancels in x_ui - x_uj)

    def _l2(self):
        return self.reg_pen

    def _rng(self):
        dev = self.user_emb.device
        if self.sampler_rng is None:
            self.sampler_rng = ops.DropoutState(self._seed, device=dev)
        elif self.sampler_rng.device != dev:
            self.sampler_rng.to(dev)
        return self.sampler_rng

    def sample(self, users):
        """neg [B, n_neg]: fresh negatives for users [B]; advances sampler_rng (on the device: nothing synchronises)."""
        if self.user_items is None:
            raise ValueError("BPR.sample: the model was built without user_items")
        rng = self._rng()
        neg = ops.neg_sample(users.to(device=self.user_emb.device, dtype=torch.int64).reshape(-1), self.user_items, self.n_neg, rng)
        rng.advance()
        return neg

    def forward(self, users, pos, neg=None):
        """-> x_ui - x_uj [B, n_neg]; one score launch over ids = [u | pos | neg]."""
        dev = self.user_emb.device
        users = users.to(device=dev, dtype=torch.int64).reshape(-1, 1)
        pos = pos.to(device=dev, dtype=torch.int64).reshape(-1, 1)
        if neg is None:
            neg = self.sample(users.reshape(-1))
        neg = neg.to(device=dev, dtype=torch.int64).reshape(users.shape[0], -1)
        ids = torch.cat([users, pos, neg], dim=1)
        self._last_ids = ids
        s = self._scores(ids)
        return s[:, :1] - s[:, 1:]

    def create_loss(self, diff, ids=None):
        """mean(-log sigmoid(diff)) + reg_pen * (l2 terms of the rows the forward that made diff looked up)."""
        ids = self._last_ids if ids is None else ids
        return -nn.functional.logsigmoid(diff).mean() + self._reg(ids, self.reg_pen)

    @torch.no_grad()
    def score_blocks(self, users, items):
        """users [B], items [B, C] -> scores [B, C]; its flattened result is what metrics.GroupedMetrics.update_blocks(scores, block=C,
        positive_index=0) takes for blocks of one positive and C - 1 negatives (metrics/NCF_evaluation/ndcg_hr_mrr.py)."""
        dev = self.user_emb.device
        users = users.to(device=dev, dtype=torch.int64).reshape(-1, 1)
        items = items.to(device=dev, dtype=torch.int64).reshape(users.shape[0], -1)
        return self._scores(torch.cat([users, items], dim=1))

    def fused_sparse_adagrad(self, lr, initial_accumulator_value=0.1):
        """ops.SparseAdagrad (sorted) over TableSet([P] + [Q] * (1 + n_neg)) and over TableSet([bu] + [bi] * (1 + n_neg)): an item that is
        positive in one sample and negative in another takes ONE step with the sum of its gradients."""
        return self._fused_adagrad(1 + self.n_neg, lr, initial_accumulator_value)

    def fused_sparse_adam(self, beta1=0.9, beta2=0.999, eps=1e-8, clip_norm=0.0):
        """ops.SparseAdam(shared=True) over the row set where SparseAdam.covers it; the biases keep their sparse .grad (K = 1)."""
        return self._fused_adam(1 + self.n_neg, beta1, beta2, eps, clip_norm)
