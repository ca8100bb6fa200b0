"""GPU: train_yolov3.py --device_metric end to end.  The run's own validation uses the device metric; the
returned network is then validated again on the same loader with either metric, and the two must agree exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import eval_oracle as E

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")]

COMMON = ["--batch_size", "4", "--data_shape", "64", "--epochs", "1", "--synthetic_samples", "8", "--save_prefix", "0000",
          "--no_random_shape", "--num_workers", "0", "--log_interval", "1"]


def _validation_block(log):
    """the last '[Epoch e] Validation:' block of a training log: its 'name=value' lines"""
    lines = log.splitlines()
    at = max(i for i, ln in enumerate(lines) if "] Validation:" in ln)
    out = []
    for ln in lines[at + 1:]:
        if "=" not in ln or ln.startswith("[") or ln.startswith("End "):
            break
        out.append(ln.strip())
    return out


@pytest.mark.parametrize("flags", [[], ["--dataset", "vid", "--window", "5,1", "--temp", "--mult_out"]], ids=["single", "mult_out"])
def test_train_script_device_metric_equals_the_host_metric(tmp_path, monkeypatch, flags):
    import train_yolov3 as T
    from viddet_amd.metrics import DeviceVOCMApMetric, DeviceVOCMApMetricTemporal, VOCMApMetric, VOCMApMetricTemporal
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("VD_AUTOTUNE", "0")
    net = T.main(COMMON + ["--device_metric"] + flags)
    (log,) = [p for p in (tmp_path / "models" / "experiments" / "0000").iterdir() if p.name.endswith("_train.log")]
    block = _validation_block(log.read_text())
    # the same validation loader again (main() closed its own), the returned network, either metric
    train_ds, val_ds, dev_metric = T.get_dataset(T.FLAGS.dataset, T.FLAGS.dataset_val)
    _, val_loader = T.get_dataloader(train_ds, val_ds, T.FLAGS.data_shape, T.FLAGS.batch_size, 0, 1)
    try:
        temporal = bool(flags)
        assert type(dev_metric) is (DeviceVOCMApMetricTemporal if temporal else DeviceVOCMApMetric)
        host_metric = (VOCMApMetricTemporal(5, 0.5, val_ds.classes) if temporal else VOCMApMetric(0.5, val_ds.classes))
        names_d, vals_d = T.validate(net, val_loader, dev_metric, T.FLAGS.data_shape)
        count_d = T.validate.last_count
        names_h, vals_h = T.validate(net, val_loader, host_metric, T.FLAGS.data_shape)
        assert count_d == T.validate.last_count == len(val_ds)
    finally:
        val_loader.close()
    assert names_d == names_h
    assert np.array_equal(np.asarray(vals_d, np.float64), np.asarray(vals_h, np.float64), equal_nan=True), (vals_d, vals_h)
    pairs = list(zip(dev_metric._per_t, host_metric._per_t)) if temporal else [(dev_metric, host_metric)]
    for a, b in pairs:
        E.assert_same_metric(a, b)
        assert sum(len(v) for v in a._scores.values()) > 0                    # the network detected something: records exist
    # what the run itself logged is this validation
    assert block == ["{}={}".format(k, v) for k, v in zip(names_d, vals_d)], block[-3:]


def _run_ranks(args, cwd, world, port):
    """train_yolov3.py as `world` processes (gloo, all on the one GPU: RCCL refuses two ranks on a device)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), VD_DIST_BACKEND="gloo", VD_AUTOTUNE="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "train_yolov3.py")] + args, cwd=cwd, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=900) for p in procs]
    return [(p.returncode, o, e) for p, (o, e) in zip(procs, outs)]


def test_train_script_device_metric_two_ranks_log_the_one_rank_validation(tmp_path, monkeypatch):
    """Two ranks match their own shards and exchange the records: what the run logs is the validation ONE process computes
    for the same network with the host metric.  The one-rank lines cannot come from a one-rank training run - its network is
    another one (the augmentation is seeded per rank, SyncBN sees other batches) - so they are computed here: the two-rank
    run's last checkpoint, validated in this process over the whole set at the ranks' batch size with a plain VOCMApMetric."""
    import train_yolov3 as T
    from viddet_amd.metrics import VOCMApMetric
    args = COMMON + ["--device_metric", "--syncbn"]
    res = _run_ranks(args, str(tmp_path), 2, 29583)
    assert all(rc == 0 for rc, _, _ in res), [e[-1200:] for _, _, e in res]
    pre = tmp_path / "models" / "experiments" / "0000"
    log = (pre / "yolo3_darknet53_voc_train.log").read_text()
    assert "End Val: # samples: 8" in log
    two = _validation_block(log)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("VD_AUTOTUNE", "0")
    old = T.FLAGS
    try:
        T.FLAGS = T.parse_flags(COMMON + ["--syncbn"])
        T.FLAGS.window = [int(v) for v in T.FLAGS.window]
        train_ds, val_ds, host_metric = T.get_dataset(T.FLAGS.dataset, T.FLAGS.dataset_val)
        assert type(host_metric) is VOCMApMetric
        net, _ = T.get_net(train_ds.classes, (0, 1))
        net.load_parameters(str(pre / "yolo3_darknet53_voc_0001.params"))        # saved after the epoch that logged `two`
        _, val_loader = T.get_dataloader(train_ds, val_ds, T.FLAGS.data_shape, 2, 0, 1)
        try:
            names, vals = T.validate(net, val_loader, host_metric, T.FLAGS.data_shape)
        finally:
            val_loader.close()
    finally:
        T.FLAGS = old
    one = ["{}={}".format(k, v) for k, v in zip(names, vals)]
    assert one[-1].startswith("mAP=") and len(one) == len(val_ds.classes) + 1
    assert sum(len(v) for v in host_metric._scores.values()) > 0
    assert two == one, [(a, b) for a, b in zip(two, one) if a != b][:4]
