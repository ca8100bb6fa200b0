"""fp64 NumPy restatement of class-agnostic detection (--model_agnostic).  TEST INFRASTRUCTURE ONLY.

Follows, under /root/reference (MXNet runs nowhere here: parity is unpinned, as oracle/ops.py states for every operator):
  yolo3.py:172-177    the box arithmetic - shared with the per-class rows, so oracle/yolo.py's yolo_output supplies it
  yolo3.py:179-182    `if autograd.is_training(): return ...` sits IN FRONT of the agnostic branch: training is untouched
  yolo3.py:184-188    YOLOOutputV3(agnostic=True): ids = confidence * 0 + arange(0, 1) -> 0 for every anchor, the score is
                      `confidence` = sigmoid(objness) (class_score is never used), rows reshaped to (B, HW*3, 6):
                      [pixel][anchor] of one head
  yolo3.py:1195-1206  the heads' rows concatenated in output order (stride 32, 16, 8), F.contrib.box_nms(overlap_thresh,
                      valid_thresh=0.01, topk, id_index=0, score_index=1, coord_start=2, force_suppress=False), slice_axis
                      to post_nms: with one id, plain NMS over the image
  wrappers.py:101-103, yolo3.py:1042-1044   yolo3_darknet53(..., agnostic=) reaches every YOLOOutputV3 of YOLOV3T
  detect_yolo3.py:797-798, 861-862, 893, 922-925   --model_agnostic: sets metric_agnostic, pred_ag, the `_ag` result name
The decode and the NMS are oracle/yolo.py's own (yolo_output, box_nms, detect_postprocess); nothing is restated twice.
"""
import numpy as np

from oracle import yolo as Y
from oracle.ops import sigmoid


def agnostic_output(pred, num_class, anchors, stride):
    """pred (B, 3*(5+C), H, W) -> (B, H*W*3, 6) rows [0, sigmoid(obj), x1, y1, x2, y2] ordered [pixel][anchor]."""
    bbox, _rc, _rs, objness, _cls = Y.yolo_output(pred, num_class, anchors, stride, training=True)   # :172-177 (bbox (B,HW*3,4))
    b = pred.shape[0]
    conf = sigmoid(objness).reshape(b, -1, 1)                                                        # :174
    ids = conf * 0.0                                                                                # :185
    return np.concatenate([ids, conf, bbox], axis=-1)                                               # :186-187


def agnostic_detect(heads, num_class, nms_thresh=0.45, nms_topk=400, post_nms=100):
    """heads: the three prediction-conv outputs (B, 3*(5+C), g, g) in output order.
    Returns ((ids (B,post,1), scores (B,post,1), bboxes (B,post,4), rows (B,post)), all rows (B,P,6))."""
    dets = [agnostic_output(h, num_class, Y.OUT_ANCHORS[s], Y.OUT_STRIDES[s]) for s, h in enumerate(heads)]
    return Y.detect_postprocess(dets, nms_thresh, nms_topk, post_nms), np.concatenate(dets, axis=1)


def per_class_detect(heads, num_class, nms_thresh=0.45, nms_topk=400, post_nms=100):
    """the per-class tail on the same heads (oracle.net.Net.detect's second half), for contrast"""
    dets = [Y.yolo_output(h, num_class, Y.OUT_ANCHORS[s], Y.OUT_STRIDES[s], training=False) for s, h in enumerate(heads)]
    return Y.detect_postprocess(dets, nms_thresh, nms_topk, post_nms), np.concatenate(dets, axis=1)


def net_detect(onet, x, nms_thresh=0.45, nms_topk=400, post_nms=100):
    """An oracle network (oracle.net.Net or a subclass) with the agnostic tail: its inference-mode heads, then the above."""
    heads = [h.v for h in onet.features(x, train=False)]
    (ids, sc, bx, rows), _ = agnostic_detect(heads, onet.C, nms_thresh, nms_topk, post_nms)
    return ids, sc, bx, rows, heads


def sweep_pairs(alldet, nms_thresh=0.45, valid_thresh=0.01, topk=400):
    """What the greedy sweep of box_nms decides on, per image: (sorted top-k scores, the score below them or None, the IoUs
    of every pair (kept row i, still-alive row j behind it) it compares).  For tie-proofing a fixture: a decision can differ
    between fp32 and fp64 only where one of these sits within round-off of its threshold or of its neighbour."""
    out = []
    for d in alldet:
        valid = np.nonzero(d[:, 1] > valid_thresh)[0]
        order = valid[np.argsort(-d[valid, 1], kind='stable')]
        nxt = d[order[topk], 1] if len(order) > topk else None
        order = order[:topk]
        bx = d[order, 2:6]
        area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
        alive = np.ones(len(order), dtype=bool)
        ious = []
        for i in range(len(order)):
            if not alive[i]:
                continue
            j = np.arange(i + 1, len(order))
            j = j[alive[j]]
            if len(j) == 0:
                continue
            iw = np.maximum(0.0, np.minimum(bx[i, 2], bx[j, 2]) - np.maximum(bx[i, 0], bx[j, 0]))
            ih = np.maximum(0.0, np.minimum(bx[i, 3], bx[j, 3]) - np.maximum(bx[i, 1], bx[j, 1]))
            inter = iw * ih
            union = area[i] + area[j] - inter
            iou = np.where(union <= 0, 0.0, inter / np.where(union <= 0, 1.0, union))
            ious.append(iou)
            alive[j[iou > nms_thresh]] = False
        out.append((d[order, 1], nxt, np.concatenate(ious) if ious else np.zeros(0)))
    return out
