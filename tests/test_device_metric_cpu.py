"""CPU: the device metric's formulation and bookkeeping without a GPU.

tests/eval_oracle.py::match_reference restates vd_voc_match's contract in the parallel first-claimant form.  Fed through
DeviceVOCMApMetric's get()-side code it must give the dictionaries and the get() VOCMApMetric gives on the same float32 arrays -
which proves the formulation and the record ordering; the kernel itself is held to the host metric in
tests/test_device_metric_gpu.py.  Also here: gather() over gloo, the ValueErrors, the flag's default."""
import os
import socket

import numpy as np
import pytest
import torch

from tests import eval_oracle as E
from viddet_amd.metrics import (DeviceVOCMApMetric, DeviceVOCMApMetricTemporal, VOCMApMetric, VOCMApMetricTemporal)

warn = pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")


def _feed(metric, case, sample_ids=None, thresh=0.5):
    rec = E.match_reference(case["ids"], case["scores"], case["boxes"], case["gt"], case["clip"], thresh, metric.num_labels)
    B = len(case["ids"])
    metric.add_records(np.arange(B) if sample_ids is None else sample_ids, *rec)


@warn
@pytest.mark.parametrize("name", sorted(E.fixed_cases()))
def test_reference_equals_host_metric_on_the_fixed_cases(name):
    case = E.fixed_cases()[name]
    dev = DeviceVOCMApMetric(0.5, E.NAMES)
    _feed(dev, case)
    E.assert_same_metric(dev, E.host_metric([case]))


def test_fixed_cases_hold_what_they_are_named_for():
    """the codes, written out: a wrong case would prove nothing on either side"""
    F = E.fixed_cases()
    hit = lambda n: E.match_reference(F[n]["ids"], F[n]["scores"], F[n]["boxes"], F[n]["gt"], F[n]["clip"], 0.5)[2].tolist()
    assert hit("two_on_one") == [[1, 0], [0, 1], [1, 0]]
    assert hit("difficult_twice") == [[-1, -1, 1]]
    assert hit("absent_classes") == [[0, 0, 1]]
    assert hit("gt_all_padded") == [[0, 0]] and hit("no_gt_rows") == [[0, 0], [0, -2]]
    assert hit("dets_all_padded") == [[-2, -2, -2]]
    assert hit("padded_in_the_middle") == [[0, -2, 1, -2, 1]]
    assert hit("iou_at_threshold") == [[1], [0]]
    assert hit("equal_iou_first_row") == [[1], [-1]]
    with np.errstate(invalid="ignore"):
        assert hit("clip") == [[1, 1, 1, 0]] and hit("no_clip") == [[1, 1, 1]]


@warn
@pytest.mark.parametrize("N", E.RANDOM_N)
@pytest.mark.parametrize("M", E.RANDOM_M)
def test_reference_equals_host_metric_on_random_cases(N, M):
    case = E.random_case(N, M, E.SEEDS.get((N, M), 0))
    E.assert_covers(case, N)
    dev = DeviceVOCMApMetric(0.5, E.NAMES)
    _feed(dev, case)
    E.assert_same_metric(dev, E.host_metric([case]))


@warn
def test_records_are_filed_in_sample_order_whatever_the_call_order():
    """three calls with out-of-order sample ids, a different N per call and scores tied across images"""
    cases = [E.random_case(7, 5, 2), E.random_case(100, 5, 0), E.random_case(7, 65, 0)]
    sids = [np.array([7, 2, 5]), np.array([0, 8, 3]), np.array([6, 1, 4])]
    dev = DeviceVOCMApMetric(0.5, E.NAMES)
    for c, s in zip(cases, sids):
        _feed(dev, c, s)
    host = VOCMApMetric(0.5, E.NAMES)
    where = sorted((int(s), k, b) for k, sid in enumerate(sids) for b, s in enumerate(sid))
    for _, k, b in where:
        c = cases[k]
        E.host_update(host, c["ids"], c["scores"], c["boxes"], c["gt"], c["clip"], order=[b])
    E.assert_same_metric(dev, host)
    dev.reset()
    assert not dev._host and dev._host_counts is None and not dev._scores and np.isnan(dev.get()[1][-1])


@warn
def test_difficult_only_class_is_present_like_on_the_host():
    """a class met only as a difficult row, never detected: the host files it with npos 0 and an empty score list"""
    case = E._case(ids=[[0]], scores=[[0.5]], boxes=[[[0, 0, 10, 10]]], gt=[[[0, 0, 10, 10, 0, 0], [20, 20, 30, 30, 2, 1]]])
    dev = DeviceVOCMApMetric(0.5, E.NAMES)
    _feed(dev, case)
    host = E.host_metric([case])
    assert 2 in host._npos and host._npos[2] == 0
    E.assert_same_metric(dev, host)


@warn
def test_class_map_and_label_ids_outside_the_table():
    """class_map: the ids are mapped on the host by the host metric's expression (a padded row becomes class_map[-1]); a
    detection id beyond num_labels is recorded like any other, a label id beyond it is left out of npos"""
    cmap = [2, -1, 0, 1]
    case = E.random_case(7, 5, 2)
    dev = DeviceVOCMApMetric(0.5, E.NAMES, class_map=cmap)
    assert dev.num_labels == 4
    lab = case["gt"].copy()
    lab[..., 4] = np.array([cmap[int(l)] for l in lab[..., 4].reshape(-1)], np.float32).reshape(lab.shape[:-1])
    dev.add_records(np.arange(3), *E.match_reference(case["ids"], case["scores"], case["boxes"], lab, case["clip"], 0.5, 4))
    host = VOCMApMetric(0.5, E.NAMES, class_map=cmap)
    E.host_update(host, case["ids"], case["scores"], case["boxes"], case["gt"], case["clip"])
    E.assert_same_metric(dev, host)
    rec = E.match_reference(np.float32([[9, 0]]), np.float32([[0.5, 0.4]]), np.float32([[[0, 0, 4, 4], [0, 0, 4, 4]]]),
                            np.float32([[[0, 0, 4, 4, 9], [0, 0, 4, 4, 0]]]), None, 0.5, 4)
    assert rec[0].tolist() == [[9, 0]] and rec[2].tolist() == [[1, 1]] and rec[3].tolist() == [1, 0, 0, 0]


@warn
def test_temporal_records_go_to_their_frame_offset():
    t = 3
    per_t = [E.random_case(7, 5, 2), E.random_case(7, 5, 3), E.random_case(7, 5, 4)]
    dev = DeviceVOCMApMetricTemporal(t, 0.5, E.NAMES)
    for j, c in enumerate(per_t):
        _feed(dev._per_t[j], c)
    host = VOCMApMetricTemporal(t, 0.5, E.NAMES)
    stack = lambda k: np.stack([c[k] for c in per_t], axis=1)
    boxes = np.clip(stack("boxes"), 0, 100)
    gt = stack("gt")
    host.update(boxes, stack("ids"), stack("scores"), gt[..., :4], gt[..., 4:5], gt[..., 5:6])
    (na, va), (nb, vb) = dev.get(), host.get()
    assert na == nb and np.array_equal(np.asarray(va), np.asarray(vb), equal_nan=True)
    for a, b in zip(dev._per_t, host._per_t):
        E.assert_same_metric(a, b)


def test_what_the_kernel_does_not_take_is_refused_by_name():
    from viddet_amd import ops
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)
    outs = lambda n: (z(1, n, dt=torch.int32), z(1, n), z(1, n, dt=torch.int8), z(4, dt=torch.int32))
    with pytest.raises(ValueError, match=r"N=1025 detections"):
        ops.voc_match(z(1, 1025), z(1, 1025), z(1, 1025, 4), z(1, 3, 5), -1, 0.5, *outs(1025))
    with pytest.raises(ValueError, match=r"M=513 label rows"):
        ops.voc_match(z(1, 8), z(1, 8), z(1, 8, 4), z(1, 513, 5), -1, 0.5, *outs(8))
    with pytest.raises(ValueError, match=r"gt must be \(B,M,5\|6\)"):
        ops.voc_match(z(1, 8), z(1, 8), z(1, 8, 4), z(1, 3, 4), -1, 0.5, *outs(8))
    m = DeviceVOCMApMetric(0.5, E.NAMES)
    with pytest.raises(ValueError, match=r"N=1025 detections .*bboxes"):
        m.update_device(z(1, 1025, 1), z(1, 1025, 1), z(1, 1025, 4), np.zeros((1, 3, 5), np.float32))
    with pytest.raises(ValueError, match=r"M=513 label rows .*labels"):
        m.update_device(z(1, 8, 1), z(1, 8, 1), z(1, 8, 4), np.zeros((1, 513, 5), np.float32))
    with pytest.raises(ValueError, match=r"labels must end in 5 .* got 7"):
        m.update_device(z(1, 8, 1), z(1, 8, 1), z(1, 8, 4), np.zeros((1, 3, 7), np.float32))
    mt = DeviceVOCMApMetricTemporal(2, 0.5, E.NAMES)
    with pytest.raises(ValueError, match=r"labels must end in 5 .* got 4"):
        mt.update_device(z(1, 2, 8, 1), z(1, 2, 8, 1), z(1, 2, 8, 4), np.zeros((1, 2, 3, 4), np.float32))
    assert not m._dev and not mt._per_t[0]._dev


def test_modules_import_on_their_own_in_a_fresh_interpreter():
    """viddet_amd.device_metric is importable first, and ops.voc_match's checks run in a program that never imported
    viddet_amd.metrics; the classes are still handed out by viddet_amd.metrics"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    progs = [
        "import viddet_amd.device_metric as D, viddet_amd.metrics as M\n"
        "assert M.DeviceVOCMApMetric is D.DeviceVOCMApMetric and M.DeviceVOCMApMetricTemporal is D.DeviceVOCMApMetricTemporal\n"
        "from viddet_amd.metrics import DeviceVOCMApMetric\n",
        "import sys, torch\nfrom viddet_amd import ops\n"
        "assert 'viddet_amd.metrics' not in sys.modules and 'viddet_amd.device_metric' not in sys.modules\n"
        "z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)\n"
        "for n, m, text in ((1025, 3, 'N=1025'), (8, 513, 'M=513')):\n"
        "    try:\n"
        "        ops.voc_match(z(1, n), z(1, n), z(1, n, 4), z(1, m, 5), -1, 0.5, z(1, n, dt=torch.int32), z(1, n),\n"
        "                      z(1, n, dt=torch.int8), z(4, dt=torch.int32))\n"
        "    except ValueError as e:\n"
        "        assert text in str(e), e\n"
        "    else:\n"
        "        raise SystemExit('not refused')\n"
        "assert 'viddet_amd.metrics' not in sys.modules\n",
        "from viddet_amd.metrics import DeviceVOCMApMetricTemporal, VOCMApMetricTemporal\n"
        "assert issubclass(DeviceVOCMApMetricTemporal, VOCMApMetricTemporal)\n",
    ]
    for prog in progs:
        r = subprocess.run([sys.executable, "-c", prog], cwd=root, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (prog, r.stderr[-1500:])


def test_library_entry_point_refuses_bad_arguments():
    """the C entry point's own checks (they run before any launch, so without a GPU)"""
    from viddet_amd import lib as L
    lib = L.load()
    assert lib.vd_abi_version() == L.ABI_VERSION                                       # an entry point was only added
    buf = torch.zeros(64, dtype=torch.float32)
    p = L.ptr(buf)
    call = lambda B, N, M, w, C, npos=p: lib.vd_voc_match(p, p, p, B, N, p, M, w, -1.0, 0.5, p, p, p, npos, None, C, None)
    for args, text in (((1, 1025, 1, 5, 4), b"N=1025"), ((1, 1, 513, 5, 4), b"M=513"), ((1, 1, 1, 4, 4), b"gt_w"),
                       ((1, 1, 1, 5, 0), b"C >= 1"), ((-1, 1, 1, 5, 4), b"B, N, M"), ((1, 1, 1, 5, 4, None), b"npos")):
        assert call(*args) != 0
        err = lib.vd_last_error()
        assert err.startswith(b"vd_voc_match:") and text in err, (args, err)
    assert call(0, 7, 3, 5, 4) == 0                                                    # no image: nothing is launched


def test_flag_is_off_by_default_and_builds_the_device_classes():
    import train_yolov3 as T
    assert T.parse_flags([]).device_metric is False
    old = T.FLAGS
    try:
        for argv, cls in (([], VOCMApMetric), (["--device_metric"], DeviceVOCMApMetric),
                          (["--device_metric", "--dataset", "vid", "--window", "3,1", "--mult_out"], DeviceVOCMApMetricTemporal)):
            T.FLAGS = T.parse_flags(argv + ["--synthetic_samples", "4"])
            T.FLAGS.window = [int(s) for s in T.FLAGS.window]
            metric = T.get_dataset(T.FLAGS.dataset, T.FLAGS.dataset_val)[2]
            assert type(metric) is cls, (argv, type(metric))
    finally:
        T.FLAGS = old


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from viddet_amd import dist as vd
    vd.init_from_env(backend="gloo")
    try:
        import warnings
        warnings.simplefilter("ignore", RuntimeWarning)
        cases = [E.random_case(7, 5, 2), E.random_case(100, 65, 0), E.random_case(7, 1, 0)]     # 9 images in 3 batches
        sid = np.arange(9).reshape(3, 3)
        mine = DeviceVOCMApMetric(0.5, E.NAMES)
        for k, c in enumerate(cases):                     # the loader's sharding: this rank's images of every batch
            own = [b for b in range(3) if sid[k, b] % world == rank]
            if own:
                part = {key: (c[key][own] if key != "clip" else c[key]) for key in c}
                _feed(mine, part, sid[k, own])
        n = mine.gather()
        assert n == 9, n
        E.assert_same_metric(mine, E.host_metric(cases))
        # the Temporal class: t record sets, ONE exchange
        calls, real = [], vd.all_gather_objects
        vd.all_gather_objects = lambda obj, group=None: (calls.append(1), real(obj, group))[1]
        try:
            tm = DeviceVOCMApMetricTemporal(2, 0.5, E.NAMES)
            for j, per in enumerate((cases, cases[::-1])):
                for k, c in enumerate(per):
                    own = [b for b in range(3) if sid[k, b] % world == rank]
                    if own:
                        _feed(tm._per_t[j], {key: (c[key][own] if key != "clip" else c[key]) for key in c}, sid[k, own])
            assert tm.gather() == 9 and len(calls) == 1, calls
        finally:
            vd.all_gather_objects = real
        E.assert_same_metric(tm._per_t[0], E.host_metric(cases))
        E.assert_same_metric(tm._per_t[1], E.host_metric(cases[::-1]))
        q.put((rank, "ok", float(mine.get()[1][-1])))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, "fail: %r %s" % (e, traceback.format_exc()[-1500:]), None))
    finally:
        dist.destroy_process_group()


def test_gather_gives_every_rank_the_single_process_metric():
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == "ok" for r in res), res
    assert res[0][2] == res[1][2] and res[0][2] > 0
