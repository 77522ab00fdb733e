"""DeepFM, ESMM and DCN with dropout restated in float64 torch on GIVEN masks: tests/model_ref64.py's layers (that file keeps dropout at 0)
with out = (x / keep_prob) * mask behind the hidden layers, in each model's order -- DeepFM dense -> dropout -> BN (deepFM.py:295-308),
ESMM dense -> dropout (ESMM.py:139-144), DCN dense -> BN -> dropout (DeepCrossNetwork.py:394-408, the last layer without BN).
masks: one [B, width] float64 0/1 tensor per hidden layer; keep_prob: fp32(1 - rate) as a Python float."""
import numpy as np
import torch

from tests import model_ref64 as M


def keep_prob(rate):
    return float(np.float32(1.0) - np.float32(rate))


def drop(x, mask, keep):
    return x / keep * mask


def tower(x, hidden, head, masks, keep):
    for (W, b), m in zip(hidden, masks):
        x = drop(M.relu(M.dense(x, W, b)), m, keep)
    return M.dense(x, *head)


def deepfm(emb, F, K, hidden, head, linear, masks, keep, bns=None, eps=1e-3):
    """bns: per hidden layer {gamma, beta} or None; TRAIN-mode batch norm on the dropped activation.  -> (logits, [(mean, var)])."""
    net, stats = emb, []
    for i, (W, b) in enumerate(hidden):
        net = drop(M.relu(M.dense(net, W, b)), masks[i], keep)
        if bns is not None:
            net, st = M.batch_norm(net, bns[i]["beta"], bns[i].get("gamma"), eps, None)
            stats.append(st)
    return M.fm_logit(emb, F, K) + M.dense(net, *head) + linear, stats


def esmm(x_ctr, x_cvr, ctr, cvr, masks_ctr, masks_cvr, keep, eps=1e-7):
    ctr_logits, cvr_logits = tower(x_ctr, ctr[0], ctr[1], masks_ctr, keep), tower(x_cvr, cvr[0], cvr[1], masks_cvr, keep)
    p = (torch.sigmoid(ctr_logits) * torch.sigmoid(cvr_logits)).clamp(eps, 1 - eps)
    return {"ctr_logits": ctr_logits, "cvr_logits": cvr_logits, "ctcvr_logits": torch.log(p / (1 - p))}


def dcn(x0, cross_w, cross_b, hidden, betas, head, masks, keep, eps=1e-3):
    """betas: the batch norms' beta, one per hidden layer but the last (None: no batch norm).  -> (logits, [(mean, var)])."""
    cross = M.cross_network(x0, cross_w, cross_b)
    net, stats = x0, []
    for i, (W, b) in enumerate(hidden):
        net = M.relu(M.dense(net, W, b))
        if betas is not None and i < len(hidden) - 1:
            net, st = M.batch_norm(net, betas[i], None, eps, None)
            stats.append(st)
        net = drop(net, masks[i], keep)
    return M.dense(torch.cat([cross, net], dim=1), *head), stats
