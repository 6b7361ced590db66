"""TEST INFRASTRUCTURE: float64 references for the training step's kernels outside BilateralSliceApply -- the up-add of
the pyramid model with its transpose (csrc/resize_bilinear.hip) and the Adam update over a flat buffer (csrc/metrics.hip).

Up-add.  `tf.image.resize_images(x, size, BILINEAR, align_corners=True)` is separable: out = Wy X Wx^T per batch and
channel, with two-tap rows.  The taps and the lerp weights are formed in FLOAT32 exactly as
``oracle.resize_bilinear_align_corners`` forms them (scale = (in - 1) / float(out - 1), src = i * scale, floor / ceil,
lerp = src - floor): like the cell coordinates of ``f64_vjps`` they are part of the op's semantics -- at index 1919 a
float64 `i * scale` lands 2.8e-4 away in the output (randn data, 960 -> 1920).  The matrices are then cast to float64 and
every sum and product is a float64 matmul.  forward = Wy X Wx^T + fine; VJP = Wy^T G Wx.

Adam.  One step of ``torch.optim.Adam``'s update (``epsilon_hat=False``) or ``tf.train.AdamOptimizer``'s
(``epsilon_hat=True``: tensorflow/python/training/adam.py, the optimizer hdrnet/bin/train.py:113 builds), in the dtype
asked for: float64 is the reference, float32 the reference optimizers' own arithmetic -- the yardstick for how far a
float32 implementation may be from the float64 value.  The hyper-parameters enter as the FLOAT32 values the C ABI
(include/hdrnet_amd_train.h) carries, widened: float32(0.999) is 0.99900001287, so `1 - beta2` is 1.3e-5 (relative)
from the double's -- an optimizer with that beta2, not a rounding error of one with 0.999.
"""
import numpy as np


# ---- bilinear resize, align_corners ----------------------------------------------------------------------------------
def resize_taps(n_in, n_out):
    """(lower, upper, lerp) of every destination index along one axis: int64, int64, float32 -- the float32 arithmetic
    of oracle.resize_bilinear_align_corners."""
    f32 = np.float32
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(n_in) / f32(n_out)
    src = (np.arange(n_out, dtype=f32) * scale).astype(f32)
    lo = np.floor(src)
    hi = np.minimum(np.ceil(src), n_in - 1)
    return lo.astype(np.int64), hi.astype(np.int64), (src - lo).astype(f32)


def resize_matrix(n_in, n_out, dtype=np.float64):
    """W [n_out, n_in]: out = W @ in along one axis.  a + (b - a) l = a (1 - l) + b l: W[i, lower] = 1 - l,
    W[i, upper] += l, the subtraction and the sum (upper == lower: an integer source coordinate, or the clamp at the far
    edge) taken in `dtype` from the float32 lerp."""
    lo, hi, l = resize_taps(n_in, n_out)
    l = l.astype(dtype)
    W = np.zeros((n_out, n_in), dtype)
    i = np.arange(n_out)
    W[i, lo] = dtype(1) - l
    W[i, hi] += l
    return W


def upsample_add_f64(coarse, fine):
    """resize(coarse [B, h, w, C] -> fine's [B, H, W, C] size) + fine, float64, one batch entry at a time."""
    B, h, w, C = coarse.shape
    _, H, W, _ = fine.shape
    Wy, Wx = resize_matrix(h, H), resize_matrix(w, W)
    out = np.empty(fine.shape, np.float64)
    for b in range(B):
        x = coarse[b].astype(np.float64)                                     # [h, w, C]
        t = np.matmul(Wx, x.transpose(0, 2, 1).reshape(h * C, w).T)          # [W, h C]
        t = np.matmul(Wy, t.T.reshape(h, C * W))                             # [H, C W]
        out[b] = t.reshape(H, C, W).transpose(0, 2, 1) + fine[b]
    return out


def upsample_vjp_f64(g, h, w, dtype=np.float64):
    """d coarse [B, h, w, C] = Wy^T G Wx of the gradient g [B, H, W, C] (d fine is g itself)."""
    B, H, W, C = g.shape
    Wy, Wx = resize_matrix(h, H, dtype), resize_matrix(w, W, dtype)
    out = np.empty((B, h, w, C), dtype)
    for b in range(B):
        x = g[b].astype(dtype)                                               # [H, W, C]
        t = np.matmul(Wy.T, x.reshape(H, W * C))                             # [h, W C]
        t = np.matmul(t.reshape(h, W, C).transpose(0, 2, 1).reshape(h * C, W), Wx)   # [h C, w]
        out[b] = t.reshape(h, C, w).transpose(0, 2, 1)
    return out


# ---- Adam ------------------------------------------------------------------------------------------------------------
def adam_hyper(lr, b1, b2, eps, dtype=np.float64):
    """The hyper-parameters as the float32 values the C ABI carries, in `dtype`."""
    return tuple(dtype(np.float32(x)) for x in (lr, b1, b2, eps))


def adam_step(p, m, v, g, t, lr, b1, b2, eps, epsilon_hat, dtype=np.float64, s=None):
    """Step number t (1-based) of Adam on arrays of `dtype` with the float32 gradient g.  Returns (p, m, v, update, s,
    unit): update = the amount subtracted from p; s = the moving average of |g| with exp_avg's weights (pass the previous
    one, or None for |m|) -- the sum of the magnitudes of exp_avg's terms, what its rounding error scales with when
    gradients of both signs cancel in it; unit = the update an element would take with exp_avg = s.

        torch       p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
        tensorflow  p -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps)
    """
    lr, b1, b2, eps = adam_hyper(lr, b1, b2, eps, dtype)
    one = dtype(1)
    g = g.astype(dtype)
    if s is None:
        s = np.abs(m)
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * (g * g)
    s = b1 * s + (one - b1) * np.abs(g)
    bc1 = one - np.power(b1, dtype(t))
    bc2 = one - np.power(b2, dtype(t))
    if epsilon_hat:
        scale = lr * np.sqrt(bc2) / bc1
        denom = np.sqrt(v) + eps
    else:
        scale = lr / bc1
        denom = np.sqrt(v) / np.sqrt(bc2) + eps
    update = scale * m / denom
    return (p - update).astype(dtype), m.astype(dtype), v.astype(dtype), update.astype(dtype), s.astype(dtype), \
        (scale * s / denom).astype(dtype)
