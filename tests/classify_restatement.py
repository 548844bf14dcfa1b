"""Plain NumPy float64 restatement of RNASeqLogisticRegression (models/polee_classify.py:13-114), what tests/test_gpu_classify.py
holds the device to.  A helper module, not a test file.

    logits = (lx - x_bias) w + z_bias
    loss   = mean over draws of loss_scale sum_s CE(labels_s, softmax(logits_s))  +  l1 sum |w|

lx_draws [D][S][n] is log expression (the log of the sampler's draws, or a point estimate with D = 1); label rows are one-hot.
"""
import numpy as np


def _logits(w, x_bias, z_bias, lx):
    return (np.asarray(lx, np.float64) - x_bias) @ w + z_bias


def _lse(z):
    mx = z.max(axis=1, keepdims=True)
    return mx[:, 0] + np.log(np.exp(z - mx).sum(axis=1))


def loss(w, x_bias, z_bias, lx_draws, labels, l1, loss_scale):
    w, x_bias, z_bias, labels = (np.asarray(a, np.float64) for a in (w, x_bias, z_bias, labels))
    total = 0.0
    for lx in lx_draws:
        z = _logits(w, x_bias, z_bias, lx)
        total += loss_scale * (labels * (_lse(z)[:, None] - z)).sum()
    return total / len(lx_draws) + l1 * np.abs(w).sum()


def loss_and_gradients(w, x_bias, z_bias, lx_draws, labels, l1, loss_scale):
    """(loss, g_w [n][k], g_x_bias [n], g_z_bias [k]); the penalty's gradient is l1 sign(w) with sign(0) = 0 (tf.abs)"""
    w, x_bias, z_bias, labels = (np.asarray(a, np.float64) for a in (w, x_bias, z_bias, labels))
    D = len(lx_draws)
    g_w, g_xb, g_zb = np.zeros_like(w), np.zeros_like(x_bias), np.zeros_like(z_bias)
    for lx in lx_draws:
        a = np.asarray(lx, np.float64) - x_bias
        z = a @ w + z_bias
        dl = (np.exp(z - _lse(z)[:, None]) - labels) * (loss_scale / D)  # (softmax - labels: rows of labels sum to 1)
        g_w += a.T @ dl
        g_xb -= w @ dl.sum(axis=0)
        g_zb += dl.sum(axis=0)
    return loss(w, x_bias, z_bias, lx_draws, labels, l1, loss_scale), g_w + l1 * np.sign(w), g_xb, g_zb


def adam_step(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-7):
    """tf.optimizers.Adam, step t = 1, 2, ...: returns (p, m, v)"""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


def predict(w, x_bias, z_bias, lx_draws):
    """predict_sample (:105-111): the mean over the draws of softmax(logits), [S][k]"""
    w, x_bias, z_bias = (np.asarray(a, np.float64) for a in (w, x_bias, z_bias))
    acc = 0.0
    for lx in lx_draws:
        z = _logits(w, x_bias, z_bias, lx)
        acc = acc + np.exp(z - _lse(z)[:, None])
    return acc / len(lx_draws)
