"""fp64 NumPy restatement of the (2+1)-D Darknet backbone of frame windows (--conv_types 21).  TEST INFRASTRUCTURE ONLY.

Follows, under /root/reference (MXNet runs nowhere here: parity is unpinned, as oracle/ops.py states for every operator):
  three_darknet.py:19-38   _conv21d: (1,3,3) Conv3D (no bias) + BN + LeakyReLU(0.1), then Conv3DRepPad depthwise (3,1,1),
                           groups = out, no bias; NO BatchNorm / activation behind it (:36)
  three_darknet.py:41-70   Conv3DRepPad: one copy of frame 0 in front, one copy of frame K-2 behind
                           (slice_axis(begin=-2, end=-1) is the frame BEFORE the last - restated as written)
  three_darknet.py:100-123 DarknetBasicBlockV3 conv_type 21: _conv3d 1x1x1, _conv21d 3, + residual
  three_darknet.py:152-226 Darknet3D: features, the temporal max pool where the 2-D stages begin (it takes an index of
                           `features`), the routes a, b, c and the extra max of a route that still carries K frames
  wrappers.py:113-130, yolo3.py:1305-1439  yolo3_3ddarknet: YOLOV3TB with k = 1 - the plain neck and heads, `d_model.` names
A window is (B,K,3,H,W); inside the trunk the frames are folded into the batch (frame b*K + t), which is what a Conv3D with
a unit time extent, a BatchNorm over (N,D,H,W) and a LeakyReLU do to them.
"""
from collections import OrderedDict

import numpy as np

from oracle import net as ON
from oracle.net import Var

LAYERS, CHANNELS = [1, 2, 8, 8, 4], [64, 128, 256, 512, 1024]


# ---- Conv3DRepPad, depthwise: x (B,C,K,h,w), w (C,1,3,1,1)
def rep_pad(x):
    return np.concatenate([x[:, :, :1], x, x[:, :, -2:-1]], axis=2)


def tdw_forward(x, w):
    K = x.shape[2]
    assert K >= 2
    xp = rep_pad(x)
    return sum(w[None, :, 0, j, 0, 0, None, None, None] * xp[:, :, j:j + K] for j in range(3))


def tdw_backward(x, w, dy):
    """(dx, dw): frame 0 also collects the front pad's gradient, frame K-2 the tail pad's"""
    K = x.shape[2]
    xp = rep_pad(x)
    dxp = np.zeros_like(xp)
    dw = np.zeros_like(w)
    for j in range(3):
        dxp[:, :, j:j + K] += w[None, :, 0, j, 0, 0, None, None, None] * dy
        dw[:, 0, j, 0, 0] = (dy * xp[:, :, j:j + K]).sum(axis=(0, 2, 3, 4))
    dx = dxp[:, :, 1:K + 1].copy()
    dx[:, :, 0] += dxp[:, :, 0]
    dx[:, :, K - 2] += dxp[:, :, K + 1]
    return dx, dw


def conv_swap(conv_types):
    """three_darknet.py:170-199: index into conv_types of the first 2-D stage (6: none)"""
    return conv_types.index(2) if 2 in conv_types else 6


def feature_plan(conv_types):
    """[(features index, kind, stage, conv type)] with kind in stem / pool / down / block"""
    out, idx, past = [(0, 'stem', -1, conv_types[0])], 1, conv_types[0]
    for gi, n in enumerate(LAYERS):
        ct = conv_types[gi + 1]
        if past == 21 and ct == 2:
            out.append((idx, 'pool', gi, 2))
            idx += 1
        out.append((idx, 'down', gi, ct))
        idx += 1
        for _ in range(n):
            out.append((idx, 'block', gi, ct))
            idx += 1
        past = ct
    if past == 21:
        out.append((idx, 'pool', 5, 2))
    return out


def param_shapes(num_class, conv_types):
    S = OrderedDict()

    def cell(name, cin, cout, k, ct, temporal):
        S[name + ".0.weight"] = (cout, cin, 1, k, k) if ct == 21 else (cout, cin, k, k)
        for t in ("gamma", "beta", "running_mean", "running_var"):
            S[name + ".1." + t] = (cout,)
        if temporal:
            S[name + ".3.conv.weight"] = (cout, 1, 3, 1, 1)

    for idx, kind, gi, ct in feature_plan(conv_types):
        nm = "d_model.features.%d" % idx
        if kind == 'stem':
            cell(nm, 3, 32, 3, ct, ct == 21)
        elif kind == 'down':
            cell(nm, CHANNELS[gi] // 2, CHANNELS[gi], 3, ct, ct == 21)
        elif kind == 'block':
            cell(nm + ".body.0", CHANNELS[gi], CHANNELS[gi] // 2, 1, ct, False)
            cell(nm + ".body.1", CHANNELS[gi] // 2, CHANNELS[gi], 3, ct, ct == 21)
    for k_, shp in ON.param_shapes(num_class).items():
        if not k_.startswith("stages."):
            S[k_] = shp
    return S


def init_params(num_class, conv_types, seed=0, obj_bias=0.0):
    rng = np.random.default_rng(seed)
    P = OrderedDict()
    for k_, shp in param_shapes(num_class, conv_types).items():
        if k_.endswith(".3.conv.weight"):
            P[k_] = 1.0 / 3 + rng.standard_normal(shp) * 0.25          # around the inflated value: the window keeps its scale
        elif k_.endswith("weight"):
            P[k_] = rng.standard_normal(shp) * np.sqrt(2.0 / int(np.prod(shp[1:])))
            if "prediction" in k_:
                P[k_] *= 0.05
        elif k_.endswith("gamma"):
            P[k_] = rng.uniform(0.2, 0.4, shp) if ".body.1.1." in k_ and k_.startswith("d_model") else rng.uniform(0.8, 1.2, shp)
        elif k_.endswith("running_var"):
            P[k_] = rng.uniform(0.8, 1.2, shp)
        elif k_.endswith("bias"):
            b = rng.standard_normal(shp) * 0.1
            b.reshape(3, -1)[:, 4] += obj_bias
            P[k_] = b
        else:
            P[k_] = rng.standard_normal(shp) * 0.1
    return OrderedDict((k_, v.astype(np.float32).astype(np.float64)) for k_, v in P.items())


class D21Net(ON.Net):
    """yolo3_3ddarknet: detect(x) / train_step(x, ...) take windows (B,K,3,H,W)."""

    def __init__(self, P, num_class, conv_types, k):
        # the per-frame cells are oracle.net's: a (O,I,1,kh,kw) weight acts on a frame as its (O,I,kh,kw) slice
        self.P5 = P
        super().__init__(OrderedDict((k_, v[:, :, 0] if (v.ndim == 5 and not k_.endswith(".3.conv.weight")) else v)
                                     for k_, v in P.items()), num_class)
        self.ct, self.k = list(conv_types), k
        self.argmax_override, self.argmax_natural = {}, {}

    def tdw(self, name, x, residual=None):
        K = self.k
        w = self.P5[name]
        n, c, h, wd = x.v.shape
        x5 = x.v.reshape(n // K, K, c, h, wd).transpose(0, 2, 1, 3, 4)
        fold = lambda a: a.transpose(0, 2, 1, 3, 4).reshape(n, c, h, wd)
        y = fold(tdw_forward(x5, w))
        if residual is not None:
            y = y + residual.v

        def bw(g):
            if residual is not None:
                residual.acc(g)
            dx5, dw = tdw_backward(x5, w, g.reshape(n // K, K, c, h, wd).transpose(0, 2, 1, 3, 4))
            self.G[name] = dw
            x.acc(fold(dx5))

        return Var(y, (x,) if residual is None else (x, residual), bw)

    def pool(self, x, name):
        """max over the K frames of (B*K,C,h,w) (TemporalGlobalMaxPool3D :73-82, F.max(axis=-3) :219,224-225)"""
        K = self.k
        v5 = x.v.reshape((-1, K) + x.v.shape[1:])
        am = v5.argmax(axis=1)
        self.argmax_natural[name] = (am, v5)
        if name in self.argmax_override:             # the device's winner (differs only at ties; cf. oracle.ops.leaky)
            am = self.argmax_override[name]
        y = np.take_along_axis(v5, am[:, None], axis=1)[:, 0]

        def bw(g):
            d5 = np.zeros_like(v5)
            np.put_along_axis(d5, am[:, None], g[:, None], axis=1)
            x.acc(d5.reshape(x.v.shape))

        return Var(y, (x,), bw)

    def cell21(self, name, x, stride, train, residual=None):
        return self.tdw(name + ".3.conv.weight", self.cell(name, x, 3, stride, train), residual)

    def backbone(self, x_bk, train):
        B, K = x_bk.shape[:2]
        assert K == self.k
        x = Var(np.asarray(x_bk, dtype=np.float64).reshape((B * K,) + x_bk.shape[2:]))
        frames, outs = K, {}
        for idx, kind, gi, ct in feature_plan(self.ct):
            nm = "d_model.features.%d" % idx
            if kind == 'stem':
                x = self.cell21(nm, x, 1, train) if ct == 21 else self.cell(nm, x, 3, 1, train)
            elif kind == 'pool':
                x, frames = self.pool(x, 'pool.trunk'), 1
            elif kind == 'down':
                x = self.cell21(nm, x, 2, train) if ct == 21 else self.cell(nm, x, 3, 2, train)
            else:
                m = self.cell(nm + ".body.0", x, 1, 1, train)
                x = self.cell21(nm + ".body.1", m, 1, train, residual=x) if ct == 21 else \
                    self.cell(nm + ".body.1", m, 3, 1, train, residual=x)
            outs[idx] = (x, frames)
        # :205-226: where the slices end
        cs = conv_swap(self.ct)
        ends = (15, 24, 29) if cs <= 4 else ((14, 24, 29) if cs == 5 else (14, 23, 29))
        routes = []
        for i, e in enumerate(ends):
            r, fr = outs[e]
            if fr > 1:
                r = self.pool(r, 'pool.route%d' % i)
            routes.append(r)
        return routes

    def train_step(self, x_bk, *targets, **kw):
        losses, G, heads = super().train_step(x_bk, *targets, **kw)
        for k_, v in list(G.items()):                # the per-frame cells' gradients back in the 5-D layout
            if self.P5[k_].ndim == 5 and v.ndim == 4:
                G[k_] = v[:, :, None]
        return losses, G, heads
