"""GPU: vd_voc_match through DeviceVOCMApMetric against the host metric.

Every comparison of this file is exact: VOCMApMetric is run image by image on the same float32 arrays (the detections clipped
as validate() clips them), and the device metric must end with EQUAL `_npos` / `_scores` / `_hits` dictionaries and an equal
get(), NaN positions included.  The outcome per detection is an integer code, so there is no tolerance to choose."""
import numpy as np
import pytest
import torch

from tests import eval_oracle as E
from viddet_amd.metrics import DeviceVOCMApMetric, DeviceVOCMApMetricTemporal, VOCMApMetric, VOCMApMetricTemporal

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")]


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _update(dev, case, sample_ids=None, labels_on_device=False):
    """as validate() calls it: the network's (B,N,1) / (B,N,1) / (B,N,4) tensors and the loader's label array"""
    dev.update_device(_d(case["ids"][..., None]), _d(case["scores"][..., None]), _d(case["boxes"]),
                      _d(case["gt"]) if labels_on_device else case["gt"], clip=case["clip"], sample_ids=sample_ids)


@pytest.mark.parametrize("name", sorted(E.fixed_cases()))
def test_fixed_cases_equal_the_host_metric(name):
    case = E.fixed_cases()[name]
    dev = DeviceVOCMApMetric(0.5, E.NAMES)
    _update(dev, case)
    E.assert_same_metric(dev, E.host_metric([case]))


def test_records_are_written_in_full_and_equal_the_reference():
    """the raw outputs of one launch on record arrays pre-filled with a pattern: every element written, and equal to the NumPy
    restatement (codes, classes, scores bit for bit, counts); label ids outside [0, C) are left out of npos"""
    from viddet_amd import ops
    case = E.random_case(257, 65, 0)
    case["gt"][0, 3, 4], case["gt"][1, 2, 4] = 4.0, 1e9                      # beyond the 4 labels: recorded nowhere
    case["ids"][2, 5] = 7.0                                                   # a detection id beyond them: recorded as it is
    B, N = case["ids"].shape
    rec_cls = torch.full((B, N), -77, dtype=torch.int32, device="cuda")
    rec_score = torch.full((B, N), float("nan"), device="cuda")
    rec_hit = torch.full((B, N), 77, dtype=torch.int8, device="cuda")
    counts = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    guard = torch.zeros(8, dtype=torch.int32, device="cuda")                 # allocated behind: stays untouched
    ops.voc_match(_d(case["ids"]), _d(case["scores"]), _d(case["boxes"]), _d(case["gt"]), case["clip"], 0.5, rec_cls, rec_score,
                  rec_hit, counts[0], counts[1])
    torch.cuda.synchronize()
    want = E.match_reference(case["ids"], case["scores"], case["boxes"], case["gt"], case["clip"], 0.5, 4)
    assert np.array_equal(rec_cls.cpu().numpy(), want[0]) and int(want[0][2, 5]) == 7
    assert np.array_equal(rec_score.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(rec_hit.cpu().numpy(), want[2])
    assert counts.cpu().numpy().tolist() == [want[3].tolist(), want[4].tolist()] and int(guard.abs().sum()) == 0
    # a second launch accumulates the counts and rewrites the same records
    ops.voc_match(_d(case["ids"]), _d(case["scores"]), _d(case["boxes"]), _d(case["gt"]), case["clip"], 0.5, rec_cls, rec_score,
                  rec_hit, counts[0], None)
    torch.cuda.synchronize()
    assert counts.cpu().numpy().tolist() == [(2 * want[3]).tolist(), want[4].tolist()]
    assert np.array_equal(rec_hit.cpu().numpy(), want[2])


@pytest.mark.parametrize("N", E.RANDOM_N)
@pytest.mark.parametrize("M", E.RANDOM_M)
def test_random_cases_equal_the_host_metric(N, M):
    case = E.random_case(N, M, E.SEEDS.get((N, M), 0))
    E.assert_covers(case, N)                          # the HOST result holds 1, 0, -1, a row claimed twice, a row without class
    dev = DeviceVOCMApMetric(0.5, E.NAMES)
    _update(dev, case, labels_on_device=(M == 5))
    E.assert_same_metric(dev, E.host_metric([case]))


def test_largest_shapes_the_kernel_takes():
    """N = 1024 and M = 512: the last element of every LDS array is in use"""
    case = E.random_case(1024, 512, 0, B=2)
    dev = DeviceVOCMApMetric(0.5, E.NAMES)
    _update(dev, case)
    E.assert_same_metric(dev, E.host_metric([case]))


def test_several_updates_out_of_order_equal_the_host_in_sample_order():
    """three calls, sample ids out of order, a different N and M per call, scores tied across images; then reset()"""
    cases = [E.random_case(7, 5, 2), E.random_case(100, 5, 0), E.random_case(7, 65, 0)]
    sids = [np.array([7, 2, 5]), np.array([0, 8, 3]), np.array([6, 1, 4])]
    dev = DeviceVOCMApMetric(0.5, E.NAMES)
    for c, s in zip(cases, sids):
        _update(dev, c, s)
    assert len(dev._dev) == 3 and not dev._host and not dev._scores          # nothing has come back before get()
    host = VOCMApMetric(0.5, E.NAMES)
    for _, k, b in sorted((int(s), k, b) for k, sid in enumerate(sids) for b, s in enumerate(sid)):
        c = cases[k]
        E.host_update(host, c["ids"], c["scores"], c["boxes"], c["gt"], c["clip"], order=[b])
    assert dev.gather() == 9                          # one process: the records come down, nothing else changes
    E.assert_same_metric(dev, host)
    E.assert_same_metric(dev, host)                   # get() again files nothing twice
    dev.reset()
    assert not dev._dev and dev._counts is None and np.isnan(dev.get()[1][-1])


def test_inputs_are_not_kept():
    """the network's outputs are plan buffers the next call overwrites: the metric reads them in its launch and keeps none"""
    case, other = E.random_case(7, 5, 2), E.random_case(7, 5, 3)
    ids, scores, boxes = _d(case["ids"][..., None]), _d(case["scores"][..., None]), _d(case["boxes"])
    dev = DeviceVOCMApMetric(0.5, E.NAMES)
    dev.update_device(ids, scores, boxes, case["gt"], clip=case["clip"])
    ids.copy_(_d(other["ids"][..., None])), scores.copy_(_d(other["scores"][..., None])), boxes.copy_(_d(other["boxes"]))
    dev.update_device(ids, scores, boxes, other["gt"], clip=other["clip"])
    E.assert_same_metric(dev, E.host_metric([case, other]))


def test_temporal_metric_files_every_frame_offset():
    """(2,3,N,.) outputs and (2,3,M,6) labels: image (b, j) goes to offset j"""
    t = 3
    per_t = [E.random_case(7, 5, 2, B=2), E.random_case(7, 5, 3, B=2), E.random_case(7, 5, 4, B=2)]
    stack = lambda k: np.ascontiguousarray(np.stack([c[k] for c in per_t], axis=1))
    ids, scores, boxes, gt = stack("ids"), stack("scores"), stack("boxes"), stack("gt")
    dev = DeviceVOCMApMetricTemporal(t, 0.5, E.NAMES)
    dev.update_device(_d(ids[..., None]), _d(scores[..., None]), _d(boxes), gt, clip=100, sample_ids=[1, 0])
    dev.update_device(_d(ids[..., None]), _d(scores[..., None]), _d(boxes), gt, clip=100, sample_ids=[3, 2])
    host = VOCMApMetricTemporal(t, 0.5, E.NAMES)
    cl = np.clip(boxes, 0, 100)
    for b in (1, 0, 1, 0):
        host.update(cl[b:b + 1], ids[b:b + 1], scores[b:b + 1], gt[b:b + 1, ..., :4], gt[b:b + 1, ..., 4:5], gt[b:b + 1, ..., 5:6])
    assert dev.gather() == 4
    (na, va), (nb, vb) = dev.get(), host.get()
    assert na == nb and "mAP t=2/3" in na and np.array_equal(np.asarray(va), np.asarray(vb), equal_nan=True)
    for a, b in zip(dev._per_t, host._per_t):
        E.assert_same_metric(a, b)


def test_update_device_neither_downloads_nor_synchronises():
    """torch's synchronisation check set to raise: a blocking copy or a stream / device synchronisation inside update_device
    would fail here (the pageable `.cuda()` upload does - it is what the check is first shown to catch)"""
    case = E.random_case(7, 5, 2)
    ids, scores, boxes = _d(case["ids"][..., None]), _d(case["scores"][..., None]), _d(case["boxes"])
    dev = DeviceVOCMApMetric(0.5, E.NAMES)
    dev.update_device(ids, scores, boxes, case["gt"], clip=case["clip"])     # first call: the counts tensor, the pinned pool
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.from_numpy(case["gt"]).cuda()
        dev.update_device(ids, scores, boxes, case["gt"], clip=case["clip"])
        dev.update_device(ids, scores, boxes, case["gt"], clip=None, sample_ids=[8, 7, 6])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(dev._dev) == 3 and not dev._host
    host = E.host_metric([case, case])
    E.host_update(host, case["ids"], case["scores"], case["boxes"], case["gt"], None, order=[2, 1, 0])
    E.assert_same_metric(dev, host)


CMAP = [2, -1, 0, 1]                                   # label id -> model id; a padded row (-1) becomes CMAP[-1] = 1, as on the host


def test_class_map_is_applied_before_the_upload_as_the_host_applies_it():
    """update_device with a class_map against VOCMApMetric(class_map=...): mapped ids, a label class mapped to -1 (dropped), and
    the padded rows of both label widths turning into class_map[-1]; num_labels follows the map; a device label tensor is
    refused beside a map (it is applied on the host)"""
    cases = [E.random_case(7, 5, 2), E.random_case(100, 65, 0), E.fixed_cases()["padded_in_the_middle"], E.fixed_cases()["gt_all_padded"]]
    dev = DeviceVOCMApMetric(0.5, E.NAMES, class_map=CMAP)
    host = VOCMApMetric(0.5, E.NAMES, class_map=CMAP)
    assert dev.num_labels == 4
    for c in cases:
        assert (c["gt"][..., 4] < 0).any()
        before = c["gt"].copy()
        _update(dev, c)
        assert np.array_equal(c["gt"], before)                               # the caller's labels are not mapped in place
        E.host_update(host, c["ids"], c["scores"], c["boxes"], c["gt"], c["clip"])
    E.assert_same_metric(dev, host)
    assert sum(host._npos.values()) > 0 and {1, 0} <= set(h for v in host._hits.values() for h in v)
    with pytest.raises(TypeError, match="class_map"):
        _update(dev, cases[0], labels_on_device=True)


def test_temporal_metric_with_a_class_map():
    t = 2
    per_t = [E.random_case(7, 5, 2, B=2), E.random_case(7, 5, 3, B=2)]
    stack = lambda k: np.ascontiguousarray(np.stack([c[k] for c in per_t], axis=1))
    ids, scores, boxes, gt = stack("ids"), stack("scores"), stack("boxes"), stack("gt")
    dev = DeviceVOCMApMetricTemporal(t, 0.5, E.NAMES, class_map=CMAP)
    dev.update_device(_d(ids[..., None]), _d(scores[..., None]), _d(boxes), gt, clip=100)
    host = VOCMApMetricTemporal(t, 0.5, E.NAMES, class_map=CMAP)
    host.update(np.clip(boxes, 0, 100), ids, scores, gt[..., :4], gt[..., 4:5], gt[..., 5:6])
    assert dev.gather() == 2
    (na, va), (nb, vb) = dev.get(), host.get()
    assert na == nb and np.array_equal(np.asarray(va), np.asarray(vb), equal_nan=True)
    for a, b in zip(dev._per_t, host._per_t):
        E.assert_same_metric(a, b)
