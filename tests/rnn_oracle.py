"""fp64 NumPy restatement of the bidirectional convolutional GRU over the K frames of a window (RNN(k, type='gru', bi=True),
/root/reference models/definitions/layers.py:267-306) and of the YOLOV3T networks built with it (--rnn_pos late | out,
yolo3.py:58-60, 152-155, 337-338, 1022-1042, 1128-1138).  TEST INFRASTRUCTURE ONLY.

MXNet is on no machine this project runs on, so the cell is restated from MXNet 1.x gluon/contrib/rnn/conv_rnn_cell.py
(Conv2DGRUCell: i2h and h2h convolutions with a bias each, 'same' size, SliceChannel(3) in the order r, z, o,
r = sigmoid(I_r + H_r), z = sigmoid(I_z + H_z), n = tanh(I_o + r * H_o), h = (1 - z) n + z h_prev, zero begin_state) and
gluon/rnn/rnn_cell.py (BidirectionalCell.unroll: l_cell over t = 0 .. K-1, r_cell over t = K-1 .. 0 with its outputs put
back in frame order, concatenated on the channel axis; layers.py:303-305 then averages the two halves)."""
from collections import OrderedDict

import numpy as np

from oracle import net_temporal as OT
from oracle import ops as R
from oracle.net import Var

CELLS = ("l_cell", "r_cell")
ARRAYS = ("i2h_weight", "h2h_weight", "i2h_bias", "h2h_bias")


def _sig(a):
    return 1.0 / (1.0 + np.exp(-a))


def _cell(xs, Wi, Wh, bi, bh, pad):
    """one direction over the frames `xs` (list of (B, Cin, h, w)) in processing order -> ([h_t], backward closure)"""
    Ch = Wh.shape[1]
    saved, outs, h = [], [], None
    for x in xs:
        I = R.conv2d(x, Wi, 1, pad, bi)
        first = h is None
        if first:                                  # begin_state: zeros, so H is the bias alone
            hp = np.zeros((x.shape[0], Ch) + x.shape[2:])
            H = np.broadcast_to(bh[None, :, None, None], I.shape)
        else:
            hp = h
            H = R.conv2d(hp, Wh, 1, pad, bh)
        r = _sig(I[:, :Ch] + H[:, :Ch])
        z = _sig(I[:, Ch:2 * Ch] + H[:, Ch:2 * Ch])
        Ho = H[:, 2 * Ch:]
        n = np.tanh(I[:, 2 * Ch:] + r * Ho)
        h = (1.0 - z) * n + z * hp
        saved.append((x, hp, r, z, n, Ho, first))
        outs.append(h)

    def bw(gs):
        G = dict(i2h_weight=np.zeros_like(Wi), h2h_weight=np.zeros_like(Wh), i2h_bias=np.zeros_like(bi), h2h_bias=np.zeros_like(bh))
        dxs, carry = [None] * len(xs), 0.0
        for s in reversed(range(len(xs))):
            x, hp, r, z, n, Ho, first = saved[s]
            dh = gs[s] + carry
            dn = dh * (1.0 - z)
            dz = dh * (hp - n)
            da = dn * (1.0 - n * n)
            dr = da * Ho
            drp, dzp = dr * r * (1.0 - r), dz * z * (1.0 - z)
            dI = np.concatenate([drp, dzp, da], axis=1)
            dH = np.concatenate([drp, dzp, da * r], axis=1)
            dxs[s], dwi = R.conv2d_backward(x, Wi, dI, 1, pad)
            G["i2h_weight"] += dwi
            G["i2h_bias"] += dI.sum(axis=(0, 2, 3))
            G["h2h_bias"] += dH.sum(axis=(0, 2, 3))                # the first step too: H was the bias there
            if first:
                carry = 0.0
            else:
                dhp, dwh = R.conv2d_backward(hp, Wh, dH, 1, pad)
                G["h2h_weight"] += dwh
                carry = dh * z + dhp
        return dxs, G

    return outs, bw


def gru(x5, P, s):
    """x5 (B, K, Cin, h, w); P['l_cell.i2h_weight'] ... ; s = 1 or 3 -> (y (B, K, Ch, h, w), bw): bw(g) -> (dx5, G) with G keyed
    like P."""
    K, pad = x5.shape[1], s // 2
    arr = lambda c: [P["%s.%s" % (c, a)] for a in ARRAYS]
    wi, wh, bi, bh = arr("l_cell")
    hl, bwl = _cell([x5[:, t] for t in range(K)], wi, wh, bi, bh, pad)
    wi, wh, bi, bh = arr("r_cell")
    hr, bwr = _cell([x5[:, t] for t in range(K - 1, -1, -1)], wi, wh, bi, bh, pad)
    y = np.stack([(hl[t] + hr[K - 1 - t]) / 2.0 for t in range(K)], axis=1)

    def bw(g):
        dl, Gl = bwl([g[:, t] / 2.0 for t in range(K)])
        dr, Gr = bwr([g[:, K - 1 - s_] / 2.0 for s_ in range(K)])
        dx = np.stack([dl[t] + dr[K - 1 - t] for t in range(K)], axis=1)
        G = {"l_cell." + a: v for a, v in Gl.items()}
        G.update({"r_cell." + a: v for a, v in Gr.items()})
        return dx, G

    return y, bw


def rnn_prefix(rnn_pos, i):
    return ("yolo_tips.%d.tip.rnn" if rnn_pos == 'late' else "yolo_outputs.%d.prediction.rnn") % i


def rnn_shapes(cin, ch, s):
    S = OrderedDict()
    for c in CELLS:
        S[c + ".i2h_weight"], S[c + ".h2h_weight"] = (3 * ch, cin, s, s), (3 * ch, ch, s, s)
        S[c + ".i2h_bias"], S[c + ".h2h_bias"] = (3 * ch,), (3 * ch,)
    return S


def param_shapes(num_class, k, rnn_pos, k_join_type='max'):
    """late: the late-join network without its tip cells (YOLODetectionNoTipBlockV3), plus a 3x3 GRU c -> 2c per scale;
    out: the per-frame network (no join in front of the heads) with a 1x1 GRU 2c -> A in place of each prediction conv."""
    S = OT.param_shapes(num_class, k, 'late', '2', k_join_type if rnn_pos == 'late' else 'max')
    A = 3 * (5 + num_class)
    for i, c in enumerate([512, 256, 128]):
        drop = ("yolo_blocks.%d.model.tip." % i) if rnn_pos == 'late' else ("yolo_outputs.%d.prediction." % i)
        for key in [key for key in S if key.startswith(drop)]:
            del S[key]
        cin, ch, s = (c, 2 * c, 3) if rnn_pos == 'late' else (2 * c, A, 1)
        for a, shp in rnn_shapes(cin, ch, s).items():
            S["%s.%s" % (rnn_prefix(rnn_pos, i), a)] = shp
    return S


def init_params(num_class, k, rnn_pos, k_join_type='max', seed=0, obj_bias=0.0):
    """oracle/net_temporal.py init_params over param_shapes above; the GRU arrays: He-scaled weights, N(0, 0.1) biases"""
    rng = np.random.default_rng(seed)
    P = OrderedDict()
    for key, shp in param_shapes(num_class, k, rnn_pos, k_join_type).items():
        if key.endswith("weight"):
            P[key] = rng.standard_normal(shp) * np.sqrt(2.0 / np.prod(shp[1:]))
            if "prediction" in key and ".rnn." not in key:
                P[key] *= 0.05
        elif key.endswith("gamma"):
            P[key] = rng.uniform(0.2, 0.4, shp) if ".body.1.1." in key and key.startswith("stages") else rng.uniform(0.8, 1.2, shp)
        elif key.endswith("running_var"):
            P[key] = rng.uniform(0.8, 1.2, shp)
        elif key.endswith("bias"):
            b = rng.standard_normal(shp) * 0.1
            if ".rnn." not in key:
                b.reshape(3, -1)[:, 4] += obj_bias
            P[key] = b
        else:
            P[key] = rng.standard_normal(shp) * 0.1
    return OrderedDict((kk, v.astype(np.float32).astype(np.float64)) for kk, v in P.items())


class RnnNet(OT.TemporalNet):
    """YOLOV3T with rnn_pos: 'late' - the GRU is the tip of each detection block, the late join follows; 'out' - the GRU is
    the prediction layer on the K per-frame tips, TemporalPooling joins its K outputs."""

    def __init__(self, P, num_class, k, rnn_pos, k_join_type):
        super().__init__(P, num_class, k, k_join_type, 'late', '2')
        assert rnn_pos in ('late', 'out') and (rnn_pos == 'late' or k_join_type in ('max', 'mean'))
        self.rnn_pos = rnn_pos

    def rnn(self, name, x, s, train):
        K = self.k
        v5 = x.v.reshape((-1, K) + x.v.shape[1:])
        Pc = {"%s.%s" % (c, a): self.P["%s.%s.%s" % (name, c, a)] for c in CELLS for a in ARRAYS}
        y5, bw5 = gru(v5, Pc, s)

        def bw(g):
            dx5, G = bw5(g.reshape(y5.shape))
            for key, v in G.items():
                self.G["%s.%s" % (name, key)] = v
            x.acc(dx5.reshape(x.v.shape))

        return Var(y5.reshape((-1,) + y5.shape[2:]), (x,), bw if train else None)

    def features(self, x_bk, train):
        stage, block, transition = OT.temporal_names(self.k, 'late', '2')
        b, K = x_bk.shape[:2]
        x = self.cell(stage(0), Var(x_bk.reshape((b * K,) + x_bk.shape[2:])), 3, 1, train)
        f = 1
        routes = []
        for nlayer, ch in zip([1, 2, 8, 8, 4], [64, 128, 256, 512, 1024]):
            x = self.cell(stage(f), x, 3, 2, train)
            f += 1
            for _ in range(nlayer):
                m = self.cell(stage(f) + ".body.0", x, 1, 1, train)
                x = self.cell(stage(f) + ".body.1", m, 3, 1, train, residual=x)
                f += 1
            if f in (15, 24, 29):
                routes.append(x)
        heads = []
        x = routes[2]
        for i in range(3):
            pre, _ = block(i)
            for j in range(5):
                x = self.cell("%s.body.%d" % (pre, j), x, 1 if j % 2 == 0 else 3, 1, train)
            if self.rnn_pos == 'late':
                tip = self.rnn(rnn_prefix('late', i), x, 3, train)
                heads.append(self.head(i, self.pool(tip, 'pool.tip%d' % i), train))
            else:
                tip = self.cell(pre + ".tip", x, 3, 1, train)
                heads.append(self.pool(self.rnn(rnn_prefix('out', i), tip, 1, train), 'pool.head%d' % i))
            if i < 2:
                t = self.cell(transition(i), x, 1, 1, train)
                x = self.upcat(t, routes[1 - i])
        return heads
