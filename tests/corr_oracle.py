"""fp64 NumPy restatement of the correlation join of a temporal window (Corr(d, k, kernal_size=1, stride=1, keep='all'),
/root/reference models/definitions/layers.py:93-132) and of the YOLOV3T networks built with it (yolo3.py:1105-1124,
1139-1140).  TEST INFRASTRUCTURE ONLY.

mx.sym.Correlation is restated from MXNet's documented operator (kernel_size 1, max_displacement = pad_size = d,
stride1 = stride2 = 1, is_multiply): the map of frame t has (2d+1)^2 channels, the vertical offset the slow index, zero
outside the map, and the sum over channels divided by kernel_size^2 * C."""
from collections import OrderedDict

import numpy as np

from oracle import net_temporal as OT
from oracle.net import Var


def corr(x5, d):
    """x5 (B, K, C, H, W) -> (y, bw): y (B, K*C + (K-1)*(2d+1)^2, H, W) = [x5 stacked | maps of t != K//2 against the
    centre frame]; bw(g) -> dx5 for an upstream gradient g of y's shape."""
    B, K, C, H, W = x5.shape
    mid, D = K // 2, 2 * d + 1
    side = [t for t in range(K) if t != mid]
    xp = np.pad(x5[:, mid], ((0, 0), (0, 0), (d, d), (d, d)))          # the centre frame, zero-padded by d
    maps = []
    for t in side:
        m = np.empty((B, D * D, H, W))
        for j in range(D * D):
            oy, ox = j // D, j % D                                          # (dy + d, dx + d)
            m[:, j] = (x5[:, t] * xp[:, :, oy:oy + H, ox:ox + W]).sum(axis=1) / C
        maps.append(m)
    y = np.concatenate([x5.reshape(B, K * C, H, W)] + maps, axis=1)

    def bw(g):
        dx = g[:, :K * C].reshape(B, K, C, H, W).copy()
        dxp = np.zeros_like(xp)
        for i, t in enumerate(side):
            gm = g[:, K * C + i * D * D:K * C + (i + 1) * D * D]
            for j in range(D * D):
                oy, ox = j // D, j % D
                dx[:, t] += gm[:, j:j + 1] * xp[:, :, oy:oy + H, ox:ox + W] / C
                dxp[:, :, oy:oy + H, ox:ox + W] += gm[:, j:j + 1] * x5[:, t] / C
        dx[:, mid] += dxp[:, :, d:d + H, d:d + W]
        return dx

    return y, bw


def corr_channels(K, C, d):
    return K * C + (K - 1) * (2 * d + 1) ** 2


def param_shapes(num_class, k, corr_pos, d):
    """The 'cat' join network's shapes with (k-1)(2d+1)^2 more input channels at every consumer of a correlation join:
    early - the first cell of each detection block; late - the prediction convs."""
    S = OT.param_shapes(num_class, k, corr_pos, '2', k_join_type='cat')
    extra = (k - 1) * (2 * d + 1) ** 2
    for i in range(3):
        key = ("yolo_blocks.%d.body.0.0.weight" % i) if corr_pos == 'early' else ("yolo_outputs.%d.prediction.weight" % i)
        s = S[key]
        S[key] = (s[0], s[1] + extra) + tuple(s[2:])
    return S


def init_params(num_class, k, corr_pos, d, seed=0, obj_bias=0.0):
    """oracle/net_temporal.py init_params over param_shapes above (same draws, same order)."""
    rng = np.random.default_rng(seed)
    P = OrderedDict()
    for key, shp in param_shapes(num_class, k, corr_pos, d).items():
        if key.endswith("weight"):
            P[key] = rng.standard_normal(shp) * np.sqrt(2.0 / np.prod(shp[1:]))
            if "prediction" in key:
                P[key] *= 0.05
        elif key.endswith("gamma"):
            P[key] = rng.uniform(0.2, 0.4, shp) if ".body.1.1." in key and key.startswith("stages") else rng.uniform(0.8, 1.2, shp)
        elif key.endswith("running_var"):
            P[key] = rng.uniform(0.8, 1.2, shp)
        elif key.endswith("bias"):
            b = rng.standard_normal(shp) * 0.1
            b.reshape(3, -1)[:, 4] += obj_bias
            P[key] = b
        else:
            P[key] = rng.standard_normal(shp) * 0.1
    return OrderedDict((kk, v.astype(np.float32).astype(np.float64)) for kk, v in P.items())


class CorrNet(OT.TemporalNet):
    """YOLOV3T with corr_pos: the 'cat' join network at the same position with the join replaced by [cat | corr maps]."""

    def __init__(self, P, num_class, k, corr_pos, d):
        super().__init__(P, num_class, k, 'cat', corr_pos, '2')
        self.d = d

    def pool(self, x, name=None):
        v5 = x.v.reshape((-1, self.k) + x.v.shape[1:])
        y, bw5 = corr(v5, self.d)

        def bw(g):
            x.acc(bw5(g).reshape(x.v.shape))

        return Var(y, (x,), bw)
