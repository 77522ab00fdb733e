"""Whole-model training steps and inference against float64 (tests/model_ref64.py) at the PRODUCT's batch routing.

The suite's conftest sets DIR_DENSE_MIN_ROWS = 1; the product runs dense.MIN_ROWS = 6144 (tests/test_gpu_dense_mid.py sets the same
literal), and a training step changes its kernel set at the batch sizes ops / dense name:

  ops.dense_small_covers   dir_dense_small_f32 gives way to dir_dense_mid_f32 (512 -> 513 rows for the 128-wide layers here; the 256-row
                           bound of the same predicate only binds from M N K > 1.2e8, i.e. layers beyond 683 x 683, which no model here has)
  ops.TOWER_MIN_ROWS       the fused inference tower switches on
  ops.dense_dw_auto_arith  its `fits_small` row bound: dW on dir_dense_dw_small_f32
  dense.MIN_ROWS           mlp_stack_supported / mlp_head_supported switch on, dir_dense_mid_f32 hands over to dir_dense_f32
  ops.DENSE_DW_MIN_ROWS    dW on dir_dense_dw_bf16x3_f32; the library's 16-slice bmm where dW stays "f32" (needs M % 16 == 0)
  ops.DENSE_BF3_MIN_ROWS   row-scaled fp16 x 2 forward, grad_bits, the carried row maxima, want_bits of units1_relu_backward

Every model runs one train() forward + its own loss + backward() with plain autograd at T - 1 and T for each of these (read from the
modules: the list follows them if they move), at one batch between the last two that is no multiple of 16, and at 100 (one of the
reference's own batch sizes).  Compared with the float64 restatement on the same values: the logits, the loss, the gradient of EVERY
parameter (sparse ones densified), the moving statistics after the step (DCN's batch norm, DIN's Dice), the eval() logits under no_grad
(the restatement's inference form), and a second step from the same parameters bit for bit.

Bars (the project's own): logits and loss 1e-5 (1 + |ref|); gradients 2e-5 of max |ref gradient| per tensor
(test_cin_stack_node_matches_float64_and_the_per_layer_nodes); dense layers' weights and biases 5e-5 of it
(test_deepfm_autograd_matches_float64); moving statistics 1e-5 (1 + |ref|).

Shapes: 8 fields x K = 16 (a 128-wide tower input), hidden 128-128 (ops.dense_auto_arith wants N >= 64 and at most a third padding),
vocabularies of a few hundred rows; DCN with one numeric column (d = 129: the padded path) and batch norm; xDeepFM with a (128, 128, 128)
CIN stack (ops.cin_stack_backward's pooled top layer, a middle layer with a bf16x3-class weight gradient, the symmetric first layer) and
a (12, 9) stack whose second layer takes the general fp32 form; DIN with
K = 64, T = 8, unit 80 / 40, tail 200 / 80, sigmoid / PReLU / Dice.

The features are kept a margin (1e-5) away from the relu / prelu kinks, where a gradient comparison between two precisions has no answer
(see build()).  Measured on an MI355X with these inputs: the worst figure of the 112 cases stands at 0.18 of its bar (DCN's logit bias
gradient at 2047 rows, 8.8e-6 of 5e-5), typical gradients at 2e-7 .. 1e-6 of the tensor's largest.

A recorder wraps every dir_* entry of the loaded library; the entry sets of the steps are asserted against the routing predicates, and
test_every_threshold_changes_some_models_entries fails if a T - 1 / T pair changes nothing (a vacuous pair must not pass)."""
import contextlib

import pytest
import torch

from tests import model_ref64 as M

pytestmark = pytest.mark.gpu

PRODUCT_MIN_ROWS = 6144      # dense.MIN_ROWS's default (the suite's environment overrides it with 1)
F, K, WIDTH, HIDDEN = 8, 16, 128, (128, 128)
VOCABS = (211, 300, 257, 199, 320, 301, 64, 500)
DIN_K, DIN_T, DIN_V, DIN_UNIT, DIN_TAIL = 64, 8, 400, (80, 40), (200, 80)
KINDS = ("deepfm", "dcn", "xdeepfm", "xdeepfm_odd", "esmm", "din_sigmoid", "din_prelu", "din_dice")


def _first(pred, lo, hi):
    for v in range(lo, hi + 1):
        if pred(v):
            return v
    raise AssertionError("no value in [%d, %d] satisfies the predicate" % (lo, hi))


def thresholds():
    """name -> T, the first batch on the far side, read from the modules' constants and predicates."""
    from dir_amd import ops
    return {
        "dense_small_covers": _first(lambda m: not ops.dense_small_covers(m, WIDTH, HIDDEN[0]), 1, ops.DENSE_SMALL_ROWS + 1),
        "TOWER_MIN_ROWS": ops.TOWER_MIN_ROWS,
        "dense_dw fits_small": _first(lambda m: ops.dense_dw_auto_arith(m, HIDDEN[1], HIDDEN[0]) == "small", 1, ops.DENSE_DW_MIN_ROWS),
        "dense.MIN_ROWS": PRODUCT_MIN_ROWS,
        "DENSE_DW_MIN_ROWS": ops.DENSE_DW_MIN_ROWS,
        "DENSE_BF3_MIN_ROWS": ops.DENSE_BF3_MIN_ROWS,
    }


def batches():
    from dir_amd import ops
    out = {100}
    for t in thresholds().values():
        out |= {t - 1, t}
    between = (ops.DENSE_DW_MIN_ROWS + ops.DENSE_BF3_MIN_ROWS) // 2 | 1
    assert ops.DENSE_DW_MIN_ROWS < between < ops.DENSE_BF3_MIN_ROWS and between % 16
    return sorted(out | {between})


BATCHES = batches()


# ---- models, parameters, features ----------------------------------------------------------------------------------------------------
def _fill(model, seed):
    """Realistic scales from a seeded generator: tables ~ N(0, 0.3), dense weights ~ 1 / sqrt(fan_in), non-zero biases, linear weights,
    PReLU / Dice alphas, batch-norm gamma / beta and moving statistics."""
    g = torch.Generator().manual_seed(seed)
    n = lambda shape, s=1.0: torch.randn(tuple(shape), generator=g) * s      # noqa: E731
    with torch.no_grad():
        for name, p in model.named_parameters():
            leaf = name.split(".")[-1]
            if "embedding_weights" in name or leaf == "table":
                v = n(p.shape, 0.3)
            elif "linear_weights" in name or leaf == "linear_bias":
                v = n(p.shape, 0.1)
            elif leaf == "alpha":
                v = 0.25 + n(p.shape, 0.1)
            elif leaf == "gamma":
                v = 1.0 + n(p.shape, 0.1)
            elif leaf in ("W1", "W2"):                       # the DIN unit's [in, out] kernels
                v = n(p.shape, p.shape[0] ** -0.5)
            elif leaf == "W3":
                v = n(p.shape, p.shape[0] ** -0.5)
            elif leaf == "cross_w":
                v = n(p.shape, p.shape[1] ** -0.5)
            elif p.dim() == 2:                               # nn.Linear [out, in], CIN [H, Hp m]
                v = n(p.shape, p.shape[1] ** -0.5)
            else:                                            # biases, beta, cross_b
                v = n(p.shape, 0.1)
            p.copy_(v.to(p.device))
        for name, b in model.named_buffers():
            if name.endswith("moving_mean"):
                b.copy_(n(b.shape, 0.2).to(b.device))
            elif name.endswith("moving_variance"):
                b.copy_((torch.rand(tuple(b.shape), generator=g) + 0.5).to(b.device))


def _mark(kind, raw):
    """The edges every case carries: duplicate ids inside the batch, pruned (-1) ids, and for DIN empty histories."""
    if kind.startswith("din"):
        raw["hist_len"][::5] = 0
        raw["cand"][1] = raw["cand"][0]
        raw["cand"][3] = -1
        raw["user"][2] = -1
        return
    ids = raw["ids"]
    ids[1] = ids[0]
    ids[::7, 2] = -1
    ids[5, 0] = -1
    ids[ids.shape[0] - 1, F - 1] = -1


def _draw(kind, raw, rows, g):
    """Fresh features for the samples `rows` (all of them when the tensors are still empty)."""
    n = rows.numel()
    if kind.startswith("din"):
        hist = torch.randint(0, DIN_V, (n, DIN_T), generator=g)
        hist[torch.rand((n, DIN_T), generator=g) < 0.1] = -1
        raw["hist"][rows] = hist
        raw["cand"][rows] = torch.randint(0, DIN_V, (n,), generator=g)
        raw["user"][rows] = torch.randint(0, 150, (n,), generator=g)
        return
    raw["ids"][rows] = torch.stack([torch.randint(0, v, (n,), generator=g) for v in VOCABS], dim=1)
    if kind == "dcn":
        raw["num"][rows] = torch.randn((n, 1), generator=g) * 0.5


def _upload(kind, raw, spec):
    """The features dict on the device from the raw tensors (spec keeps what reference() reads)."""
    if kind.startswith("din"):
        return {k: raw[k].cuda() for k in ("hist", "hist_len", "cand", "user")}
    spec["ids"] = raw["ids"].cuda()
    feats = {"C%d" % f: spec["ids"][:, f].contiguous() for f in range(F)}
    if kind == "dcn":
        feats["C4_num"] = spec["num"] = raw["num"].cuda()
    if kind == "esmm":
        feats["w_click"] = spec["w_click"] = raw["w_click"].cuda()
    return feats


KINK_MARGIN = 1e-5


def build(kind, B):
    """-> (model on cuda in train(), feats, labels, spec) for one case; everything seeded by (kind, B).

    relu and prelu have no derivative at 0, and a sample whose pre-activation lies within fp32's rounding of 0 (some 1e-6 on these O(1)
    sums of 128-256 products) may pass the gate on one side of the comparison and not on the other: both gradients are then right, each
    for its own branch, and they differ by that sample's whole share -- one flipped unit moves a table row's gradient by percents of the
    largest, since a row collects B / vocabulary samples of weight 1 / B.  With 3e6 pre-activations per step that happens in every few
    cases.  So the features are conditioned: samples with a float64 pre-activation inside KINK_MARGIN = 1e-5 of 0 (ten times that
    rounding; a few dozen of 12 288) draw fresh features until none is left.  The kernels still make every gate decision themselves."""
    from dir_amd import feature_column as fc
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + B)
    cats = [fc.categorical_column_with_identity("C%d" % f, VOCABS[f]) for f in range(F)]
    embs = [fc.embedding_column(c, K) for c in cats]
    labels = torch.randint(0, 2, (B, 1), generator=g).float().cuda()
    spec = {"kind": kind, "B": B}
    every = torch.arange(B)
    if kind.startswith("din"):
        raw = {"hist": torch.zeros((B, DIN_T), dtype=torch.int64), "cand": torch.zeros(B, dtype=torch.int64), "user": torch.zeros(B, dtype=torch.int64),
               "hist_len": torch.randint(0, DIN_T + 1, (B,), generator=g).int()}
    else:
        raw = {"ids": torch.zeros((B, F), dtype=torch.int64), "num": torch.zeros((B, 1)), "w_click": torch.rand((B, 1), generator=g) + 0.5}
    _draw(kind, raw, every, g)
    _mark(kind, raw)
    if kind == "deepfm":
        from dir_amd.deepfm import DeepFM
        model = DeepFM(linear_feature_columns=cats, dnn_feature_columns=embs, dnn_hidden_units=list(HIDDEN), fm_embedding_size=K)
    elif kind == "dcn":
        from dir_amd.dcn import DeepCrossNetwork
        # "C4_num" sorts between C4_embedding and C5_embedding: d = 129 (the padded path), two runs of embedding columns
        model = DeepCrossNetwork(columns=embs + [fc.numeric_column("C4_num")], cross_layer_num=3, dnn_hidden_units=list(HIDDEN), batch_norm=True)
    elif kind in ("xdeepfm", "xdeepfm_odd"):
        from dir_amd.xdeepfm import XDeepFM
        model = XDeepFM(linear_feature_columns=cats, dnn_feature_columns=embs, cin_layer_sizes=(128, 128, 128) if kind == "xdeepfm" else (12, 9),
                        dnn_hidden_units=HIDDEN)
    elif kind == "esmm":
        from dir_amd.esmm import ESMM
        model = ESMM(columns=embs, ctr_weight_column="w_click", dnn_hidden_units=list(HIDDEN))
        labels = {"click_label": labels, "convert_label": torch.randint(0, 2, (B, 1), generator=g).float().cuda()}
    else:
        from dir_amd.din import DIN
        act = kind.split("_")[1]
        user = fc.embedding_column(fc.categorical_column_with_identity("user", 150), 16)
        model = DIN(feature_columns=[user], item_vocab_size=DIN_V, embedding_dim=DIN_K, attention_hidden_units=DIN_UNIT,
                    attention_activation=act, attention_normalize=(act == "prelu"), dnn_hidden_units=DIN_TAIL,
                    dnn_activation_fn="relu" if act == "sigmoid" else act)
        spec.update(act=act, normalize=(act == "prelu"))
    model = model.cuda().train()
    _fill(model, 77 + KINDS.index(kind))
    # DCN's second layer reads a batch-normalised activation: fresh features for one sample move every sample's input to it by O(1 / B),
    # ten times the margin, so redrawing samples never settles there -- a unit of that layer with a near sample draws a fresh bias instead
    # (it shifts that unit alone, and nothing under it)
    coupled = {1: model.hidden[1].bias} if kind == "dcn" else {}
    for _ in range(40):
        feats = _upload(kind, raw, spec)
        with torch.no_grad(), M.kinks() as pre:
            reference(kind, model, feats, labels, spec)
        near = torch.zeros(B, dtype=torch.bool, device="cuda")
        for i, t in enumerate(pre):
            if i not in coupled:
                near |= t.abs().reshape(B, -1).min(dim=1).values < KINK_MARGIN
        rows = near.nonzero().reshape(-1).cpu()
        if rows.numel():
            _draw(kind, raw, rows, g)
            _mark(kind, raw)
            continue
        units = {i: (pre[i].abs().min(dim=0).values < KINK_MARGIN).nonzero().reshape(-1) for i in coupled}
        if not any(u.numel() for u in units.values()):
            return model, feats, labels, spec
        with torch.no_grad():
            for i, u in units.items():
                if u.numel():
                    coupled[i][u] = (torch.randn(u.numel(), generator=g) * 0.1).cuda()
    raise AssertionError("%s B=%d: samples still within %.0e of a relu / prelu kink" % (kind, B, KINK_MARGIN))


def _lin(l):
    return (l.weight, l.bias)


def params_of(kind, model):
    """The module's parameters in the structure reference() reads (M.flatten pairs them with the float64 leaves)."""
    if kind == "deepfm":
        return {"tabs": list(model.embedding_weights), "lws": list(model.linear_weights), "lb": model.linear_bias,
                "hidden": [_lin(l) for l in model.hidden], "head": _lin(model.logits_layer)}
    if kind == "dcn":
        return {"tabs": list(model.embedding_weights), "cross_w": model.cross_w, "cross_b": model.cross_b,
                "hidden": [_lin(l) for l in model.hidden], "beta": [b.beta for b in model.bns], "head": _lin(model.logits_layer)}
    if kind.startswith("xdeepfm"):
        return {"tabs": list(model.embedding_weights), "lws": list(model.linear_weights), "lb": model.linear_bias, "cin": list(model.cin_W),
                "cin_out": _lin(model.cin_out), "hidden": [_lin(l) for l in model.hidden], "dnn_out": _lin(model.dnn_out)}
    if kind == "esmm":
        return {t: {"tabs": list(m.input_layer.embedding_weights), "hidden": [_lin(l) for l in m.hidden], "head": _lin(m.logits)}
                for t, m in (("ctr", model.ctr_model), ("cvr", model.cvr_model))}
    a = model.attention
    P = {"table": a.table, "user": model.input_layer.embedding_weights[0], "unit": [a.W1, a.b1, a.W2, a.b2, a.W3, a.b3],
         "hidden": [_lin(l) for l in model.hidden], "head": _lin(model.logits_layer)}
    if a.activation != "sigmoid":
        P["unit_alpha"] = [a.act1.alpha, a.act2.alpha]
        P["tail_alpha"] = [m.alpha for m in model.acts]
    return P


def moving_of(kind, model):
    """[(module with moving_mean / moving_variance / momentum)] in the order reference() returns the batch statistics."""
    if kind == "dcn":
        return list(model.bns)
    if kind == "din_dice":
        return [model.attention.act1, model.attention.act2] + list(model.acts)
    return []


def reference(kind, model, feats, labels, spec, dtype=torch.float64, train=True):
    """The restatement on the module's current values -> (leaves, logits (a dict for ESMM), loss, [(batch mean, batch variance)])."""
    P = M.leaves(params_of(kind, model), dtype)
    ids = spec.get("ids")
    buf = lambda t: t.detach().to(dtype)      # noqa: E731
    emb = lambda tabs: [M.onehot(t, ids[:, f]) for f, t in enumerate(tabs)]      # noqa: E731
    stats = []
    if kind == "deepfm":
        logits, _ = M.deepfm(torch.cat(emb(P["tabs"]), dim=1), F, K, P["hidden"], P["head"], M.linear_logit(P["lws"], ids, P["lb"]))
        loss = M.weighted_loss(logits, labels, None, "sum")                      # the canned head's SUM reduction (deepFM.py:72)
    elif kind == "dcn":
        blocks = {"C%d_embedding" % f: e for f, e in enumerate(emb(P["tabs"]))}
        blocks["C4_num"] = buf(spec["num"])
        bns = [{"beta": be, "moving_mean": buf(b.moving_mean), "moving_variance": buf(b.moving_variance)} for be, b in zip(P["beta"], model.bns)]
        logits, stats = M.dcn(M.input_layer(blocks), P["cross_w"], P["cross_b"], P["hidden"], bns, P["head"], train=train, eps=model.bns[0].eps)
        loss = M.weighted_loss(logits, labels, None, "mean")                     # DeepCrossNetwork.py:209-225
    elif kind.startswith("xdeepfm"):
        logits = M.xdeepfm(torch.cat(emb(P["tabs"]), dim=1), F, K, P["cin"], P["cin_out"], P["hidden"], P["dnn_out"],
                           M.linear_logit(P["lws"], ids, P["lb"]))
        loss = M.weighted_loss(logits, labels, None, "mean")
    elif kind == "esmm":
        x = {t: torch.cat(emb(P[t]["tabs"]), dim=1) for t in ("ctr", "cvr")}     # each tower its own variables (ESMM.py:62-66)
        logits = M.esmm(x["ctr"], x["cvr"], (P["ctr"]["hidden"], P["ctr"]["head"]), (P["cvr"]["hidden"], P["cvr"]["head"]))
        loss = M.esmm_loss(logits, labels["click_label"], labels["convert_label"], ctr_weights=buf(spec["w_click"]))
    else:
        a = model.attention
        act = spec["act"]

        def acts(alphas, mods):
            if alphas is None:
                return None
            return [dict(alpha=al, **({"moving_mean": buf(m.moving_mean), "moving_variance": buf(m.moving_variance)} if act == "dice" else {}))
                    for al, m in zip(alphas, mods)]
        cols = M.onehot(P["user"], feats["user"])
        logits, us, ts = M.din(P["table"], feats["hist"], feats["hist_len"].long(), feats["cand"], P["unit"], P["hidden"], P["head"], columns=cols,
                               attention_activation=act, attention_acts=acts(P.get("unit_alpha"), [a.act1, a.act2]), normalize=spec["normalize"],
                               dnn_activation="relu" if act == "sigmoid" else act, dnn_acts=acts(P.get("tail_alpha"), list(model.acts)), train=train)
        stats = us + ts
        loss = M.weighted_loss(logits, labels, None, "mean")
    return P, logits, loss, stats


def model_loss(kind, model, feats, labels, logits):
    if kind == "deepfm":
        return model.create_loss(feats, logits, labels)[0]
    if kind == "dcn":
        return model.create_loss(feats, logits, labels)[0]
    if kind == "esmm":
        return model.get_loss(feats, labels, logits)[0]
    return torch.nn.functional.binary_cross_entropy_with_logits(logits, labels)


def _logit_dict(kind, logits):
    return {k: logits[k] for k in ("ctr_logits", "cvr_logits", "ctcvr_logits")} if kind == "esmm" else {"logits": logits}


# ---- the recorder ----------------------------------------------------------------------------------------------------------------------
_QUERIES = ("_bytes", "_partials", "_words", "_blocks")


@pytest.fixture
def recorder(built_lib, monkeypatch):
    """Wraps every dir_* launch entry of the loaded library object (as tests/test_gpu_cross.py wraps dir_cross_onehot_i64);
    `with recorder(names): ...` collects the names of the entries called inside."""
    from dir_amd import _lib
    lib = _lib.load()
    sink = [None]
    for name in _lib.SIGNATURES:
        if name in ("dir_last_error", "dir_version") or name.endswith(_QUERIES):
            continue
        real = getattr(lib, name)

        def wrapped(*a, _name=name, _real=real):
            if sink[0] is not None:
                sink[0].add(_name)
            return _real(*a)
        monkeypatch.setattr(lib, name, wrapped)

    @contextlib.contextmanager
    def into(names):
        sink[0] = names
        try:
            yield names
        finally:
            sink[0] = None
    return into


@pytest.fixture(autouse=True)
def product_routing(monkeypatch):
    from dir_amd import dense as D
    monkeypatch.setattr(D, "MIN_ROWS", PRODUCT_MIN_ROWS)
    D.reset_routing()
    yield


ENTRIES = {}      # (kind, B) -> {"train": frozenset, "eval": frozenset}: shared by the gradient cases and the straddle test


def _train_step(kind, model, feats, labels):
    for p in model.parameters():
        p.grad = None
    logits = model(feats)
    loss = model_loss(kind, model, feats, labels, logits)
    loss.backward()
    return logits, loss


def _record_entries(kind, B, recorder):
    """The entry sets of one training step and one eval() forward (no float64 work): what the straddle test needs of a case that the
    gradient tests have not already run in this process."""
    if (kind, B) not in ENTRIES:
        model, feats, labels, _ = build(kind, B)
        with recorder(set()) as tr:
            _train_step(kind, model, feats, labels)
        model.eval()
        with recorder(set()) as ev, torch.no_grad():
            model(feats)
        torch.cuda.synchronize()
        ENTRIES[(kind, B)] = {"train": frozenset(tr), "eval": frozenset(ev)}
    return ENTRIES[(kind, B)]


# ---- what the predicates say must have run ---------------------------------------------------------------------------------------------
DW_ENTRIES = {"dir_dense_dw_bf16x3_f32", "dir_dense_dw_f16x2_f32", "dir_dense_dw_f16x2_scaled_f32", "dir_dense_dw_small_f32"}
HEAD_ENTRIES = {"dir_units1_relu_backward_f32", "dir_units1_relu_backward_bits_f32"}


def dense_layers(kind):
    """[(padded in_features, out_features)] of the hidden layers that see B rows in a training step."""
    if kind == "dcn":
        return [(WIDTH + 4, HIDDEN[0]), (HIDDEN[0], HIDDEN[1])]
    if kind.startswith("din"):
        d = 16 + 2 * DIN_K
        return [(d, DIN_TAIL[0]), (DIN_TAIL[0], DIN_TAIL[1])]
    return [(WIDTH, HIDDEN[0]), (HIDDEN[0], HIDDEN[1])]


def check_entries(kind, B, model, train):
    """The dense forward and dW entries a training step at B rows must have called, from the routing predicates."""
    from dir_amd import dense as D, ops
    for Kd, N in dense_layers(kind):
        if ops.dense_auto_arith(B, Kd, N) == "bf16x3":
            want = {"dir_dense_f16x2_rows_f32", "dir_dense_bf16x3_f32"}          # (row-scaled fp16 x 2 where the rows are covered)
        elif ops.dense_small_covers(B, Kd, N):
            want = {"dir_dense_small_f32"}
        elif ops.dense_mid_covers(B, Kd, N):
            want = {"dir_dense_mid_f32"}
        else:
            want = {"dir_dense_f32"}
        assert want & train, (kind, B, Kd, N, sorted(want), sorted(train))
        dw = ops.dense_dw_auto_arith(B, N, Kd)
        if dw == "small":
            assert "dir_dense_dw_small_f32" in train, (kind, B, N, Kd, sorted(train))
        elif dw == "bf16x3":
            assert (DW_ENTRIES - {"dir_dense_dw_small_f32"}) & train, (kind, B, N, Kd, sorted(train))
            if B < ops.DENSE_BF3_MIN_ROWS and not kind.startswith("din"):      # no grad_bits under that many rows: bf16 x 3 itself
                assert "dir_dense_dw_bf16x3_f32" in train, (kind, B, sorted(train))
    if all(ops.dense_dw_auto_arith(B, N, Kd) == "f32" for Kd, N in dense_layers(kind)) and not kind.startswith(("xdeepfm", "din")):
        assert not (DW_ENTRIES & train), (kind, B, sorted(train))               # (the CIN's pooled top layer and the DIN unit's rows call dense_dw too)
    # the tower + logit layer as one node: DeepFM, xDeepFM, ESMM whole towers, DCN's last layer (dense._MlpHeadFn)
    if kind in ("deepfm", "xdeepfm", "xdeepfm_odd", "esmm", "dcn"):
        lins = list(model.ctr_model.hidden if kind == "esmm" else model.hidden)
        head = {"deepfm": lambda: model.logits_layer, "dcn": lambda: model.logits_layer, "esmm": lambda: model.ctr_model.logits}.get(
            kind, lambda: model.dnn_out)()
        x = torch.empty((B, HIDDEN[0] if kind == "dcn" else WIDTH), device="cuda")
        with torch.enable_grad():
            fused = (D.mlp_stack_supported(lins[-1:], x, torch.relu) if kind == "dcn" else D.mlp_head_supported(lins, head, x, torch.relu))
        assert fused == (B >= PRODUCT_MIN_ROWS), (kind, B, fused)
        assert bool(HEAD_ENTRIES & train) == fused, (kind, B, fused, sorted(train))
    assert all(int(k.split("x")[1]) < 16 for k in D.ROUTING["library"]), dict(D.ROUTING)      # (as test_gpu_models._check_routing)


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
def _dense_grad(g):
    return g.to_dense() if g.is_sparse else g


def _bar(path):
    """Dense layers' weights and biases 5e-5, everything else 2e-5 -- of max |reference gradient| of the tensor."""
    return 5e-5 if path.split(".")[0] in ("hidden", "head", "unit", "cin_out", "dnn_out") or ".hidden." in path or ".head." in path else 2e-5


def _same_grad(a, b):
    if a.is_sparse != b.is_sparse:
        return False
    if a.is_sparse:
        a, b = a.coalesce(), b.coalesce()
        return torch.equal(a.indices(), b.indices()) and torch.equal(a.values(), b.values())
    return torch.equal(a, b)


def run_case(kind, B, recorder, with_fp32=False):
    """One case -> [(what, error, bar)] (errors already divided by their scale), having checked the entry sets and the bitwise rerun."""
    model, feats, labels, spec = build(kind, B)
    movers = moving_of(kind, model)
    before = [(m.moving_mean.double().clone(), m.moving_variance.double().clone()) for m in movers]
    ref_P, ref_logits, ref_loss, ref_stats = reference(kind, model, feats, labels, spec)      # (reads the moving statistics' old values)
    pairs = list(zip(M.flatten(params_of(kind, model)), M.flatten(ref_P)))
    ref_grads = torch.autograd.grad(ref_loss, [r for _, (_, r) in pairs])
    with recorder(set()) as train:
        logits, loss = _train_step(kind, model, feats, labels)
    torch.cuda.synchronize()
    figures = []
    rel = lambda got, ref: float(((got.double() - ref).abs() / (1 + ref.abs())).max())      # noqa: E731
    for k, v in _logit_dict(kind, logits).items():
        figures.append(("train " + k, rel(v.detach(), _logit_dict(kind, ref_logits)[k].detach()), 1e-5))
    figures.append(("loss", rel(loss.detach(), ref_loss.detach()), 1e-5))
    grads = {}
    for ((path, p), _), rg in zip(pairs, ref_grads):
        assert p.grad is not None, (kind, B, path)
        grads[path] = p.grad
        scale = float(rg.abs().max())
        if spec.get("normalize") and path == "unit.5":
            # the softmax over the positions removes the score layer's bias from the loss: its gradient is 0 but for the rounding of
            # a sum of terms the size of that layer's weight gradient's, which is therefore its scale
            scale = float(ref_grads[[q for (q, _), _ in pairs].index("unit.4")].abs().max())
        assert scale > 0, (kind, B, path)                      # every parameter takes part in the loss
        figures.append(("grad " + path, float((_dense_grad(p.grad).double() - rg).abs().max()) / scale, _bar(path)))
    for i, (m, (mm, mv), (bm, bv)) in enumerate(zip(movers, before, ref_stats)):
        figures.append(("moving_mean %d" % i, rel(m.moving_mean, M.moving_update(mm, bm, m.momentum)), 1e-5))
        figures.append(("moving_variance %d" % i, rel(m.moving_variance, M.moving_update(mv, bv, m.momentum)), 1e-5))
    assert len(ref_stats) == len(movers)
    if with_fp32:      # fp32's own distance from float64 on the same graph (plain torch ops): printed next to the HIP path's
        P32, l32, loss32, _ = reference(kind, model, feats, labels, spec, dtype=torch.float32)
        g32 = torch.autograd.grad(loss32, [r for _, r in M.flatten(P32)])
        fp32 = {"loss": rel(loss32.detach(), ref_loss.detach())}
        for k, v in _logit_dict(kind, l32).items():
            fp32["train " + k] = rel(v.detach(), _logit_dict(kind, ref_logits)[k].detach())
        for ((path, _), _), rg, g in zip(pairs, ref_grads, g32):
            fp32["grad " + path] = float((g.double() - rg).abs().max()) / max(float(rg.abs().max()), 1e-300)
        figures = [(w, e, b, fp32.get(w)) for w, e, b in figures]
    # the same step again from the same parameters: bit for bit
    _train_step(kind, model, feats, labels)
    torch.cuda.synchronize()
    differing = [path for (path, p), _ in pairs if not _same_grad(grads[path], p.grad)]
    # inference at the same batch: eval() under no_grad against the restatement's inference form (the moving statistics as they now are)
    model.eval()
    with recorder(set()) as ev, torch.no_grad():
        got = model(feats)
    torch.cuda.synchronize()
    with torch.no_grad():
        _, ref_eval, _, _ = reference(kind, model, feats, labels, spec, train=False)
    for k, v in _logit_dict(kind, got).items():
        figures.append(("eval " + k, rel(v, _logit_dict(kind, ref_eval)[k])) + ((1e-5,) if not with_fp32 else (1e-5, None)))
    ENTRIES[(kind, B)] = {"train": frozenset(train), "eval": frozenset(ev)}
    check_entries(kind, B, model, train)
    assert not differing, "%s B=%d: gradients differ between two identical steps: %s" % (kind, B, differing)
    return figures


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_training_step_and_inference_match_float64(kind, B, recorder):
    figures = run_case(kind, B, recorder)
    for what, err, bar in figures:
        print("%s B=%d %-28s %.3e (bar %.0e)" % (kind, B, what, err, bar))
    bad = [(w, e, b) for w, e, b in figures if not e <= b]
    assert not bad, "%s B=%d: %s" % (kind, B, ", ".join("%s %.3e > %.0e" % x for x in bad))


def test_shapes_meet_the_routing_predicates(built_lib):
    """The shapes above are the smallest that keep the product kernels engaged on the far side of the thresholds: checked, not trusted."""
    from dir_amd import ops
    T = thresholds()
    big = T["DENSE_BF3_MIN_ROWS"]
    assert ops.dense_auto_arith(big, WIDTH, HIDDEN[0]) == "bf16x3" and ops.dense_auto_arith(big - 1, WIDTH, HIDDEN[0]) == "f32"
    assert ops.dense_auto_arith(big, WIDTH, 64) == "f32"                          # (why the towers are not 64 wide)
    assert ops.dense_dw_auto_arith(T["DENSE_DW_MIN_ROWS"], HIDDEN[1], HIDDEN[0]) == "bf16x3"
    assert ops.dense_dw_auto_arith(T["DENSE_DW_MIN_ROWS"] - 1, HIDDEN[1], HIDDEN[0]) == "small"
    assert ops.dense_dw_auto_arith(T["dense_dw fits_small"] - 1, HIDDEN[1], HIDDEN[0]) == "f32"
    assert ops.dense_small_covers(T["dense_small_covers"] - 1, WIDTH, HIDDEN[0]) and ops.dense_mid_covers(T["dense_small_covers"], WIDTH, HIDDEN[0])
    assert ops.dense_mid_covers(PRODUCT_MIN_ROWS - 1, WIDTH, HIDDEN[0]) and not ops.dense_mid_covers(PRODUCT_MIN_ROWS, WIDTH, HIDDEN[0])
    assert (WIDTH + 1) % 4                                                        # DCN's input width: the padded path
    assert ops.cin_dw_auto_arith(F, K, 128, 128) == "bf16x3" and ops.cin_dw_auto_arith(F, K, 12, 9) == "f32"
    assert len(BATCHES) == 2 * len(T) + 2 and all(T[k] - 1 in BATCHES and T[k] in BATCHES for k in T)


def test_cin_stack_routes(recorder):
    """ops.cin_stack_backward's routes: the (128, 128, 128) stack takes the pooled top layer, a bf16x3-class weight gradient on the middle
    layer and the symmetric kernel on the first; the (12, 9) stack's top layer takes the general fp32 form."""
    B = 100
    wide, odd = _record_entries("xdeepfm", B, recorder)["train"], _record_entries("xdeepfm_odd", B, recorder)["train"]
    print("xdeepfm:", " ".join(sorted(n for n in wide if "cin" in n)))
    print("xdeepfm_odd:", " ".join(sorted(n for n in odd if "cin" in n)))
    assert "dir_cin_pool_dx_f32" in wide and {"dir_cin_dw_sym_f16x2_f32", "dir_cin_dw_sym_bf16x3_f32"} & wide, sorted(wide)
    assert {"dir_cin_dw_bf16x3_f32", "dir_cin_dw_f16x2_f32"} & wide, sorted(wide)
    assert "dir_cin_dw_f32" in odd and "dir_cin_pool_dx_f32" not in odd and not {"dir_cin_dw_bf16x3_f32", "dir_cin_dw_f16x2_f32"} & odd, sorted(odd)


def test_every_threshold_changes_some_models_entries(recorder):
    """For every threshold some model's set of entries (training step + inference) differs between T - 1 and T rows: the pairs above really
    sit on two sides of something.  Prints the observed sets as differences along the batch list (profiles/NOTES.md holds a copy)."""
    vacuous = []
    for name, t in thresholds().items():
        for kind in KINDS:
            lo, hi = _record_entries(kind, t - 1, recorder), _record_entries(kind, t, recorder)
            if lo != hi:
                break
        else:
            vacuous.append((name, t))
    for kind in KINDS:
        prev = None
        for B in BATCHES:
            e = ENTRIES.get((kind, B))
            if e is None:
                continue
            for mode in ("train", "eval"):
                if prev is None:
                    print("%s B=%d %s: %s" % (kind, B, mode, " ".join(sorted(e[mode]))))
                elif e[mode] != prev[mode]:
                    print("%s B=%d %s: %s" % (kind, B, mode, " ".join(["+" + n for n in sorted(e[mode] - prev[mode])]
                                                                      + ["-" + n for n in sorted(prev[mode] - e[mode])])))
            prev = e
    assert not vacuous, "no model's entries change across %s" % (vacuous,)
