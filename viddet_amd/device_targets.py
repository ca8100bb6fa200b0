"""The YOLO prefetch targets of a training batch on the device.

With `device_targets=True` a training transform keeps every decision it takes today - the draws, the boxes - but does not run
`prefetch_targets`: in place of the five dense target columns and the gt column a sample carries ONE label column, the
transformed boxes themselves, (M,5) `x1, y1, x2, y2, id` (a 6th column = the mix ratio with mixup; (t,M,.) for per-frame
labels).  `Loader._collate` pads it with -1 like the gt column; `targets_on_device` uploads the batch's labels in one copy and
vd_yolo_targets (viddet_amd/csrc/vd_targets.hip) writes the dense tensors where the loss kernel reads them.

This module imports NumPy only; torch is imported by `targets_on_device`.
"""
import numpy as np

from .consts import STRIDES

MAX_GT = 512             # vd_yolo_targets takes at most this many label rows per image


def label_column(bb, mixup=False):
    """One frame's transformed boxes -> its (M,5) / (M,6) fp32 label rows: corner box, class id (column 4, as
    YOLO3VideoTrainTransform reads it), and with mixup the row's mix ratio (the last column of a MixupDetection label)."""
    b = np.asarray(bb)
    cols = [b[:, :5]] + ([b[:, -1:]] if mixup else [])
    return np.ascontiguousarray(np.concatenate(cols, axis=1), dtype=np.float32)


def num_rows(height, width):
    """P: rows of the dense targets of one image"""
    return 3 * sum((height // s) * (width // s) for s in STRIDES)


def check_labels(labels, num_class):
    """The host-side half of `targets_on_device`: (B,M,5|6) or (B,t,M,5|6) fp32 labels -> (N,M,w) with t folded into N.
    ValueError for more than MAX_GT rows and for a class id of a valid row (one before the image's first padded row) that is
    not an integer in [0, num_class)."""
    lab = np.ascontiguousarray(labels, dtype=np.float32)
    if lab.ndim not in (3, 4) or lab.shape[-1] not in (5, 6):
        raise ValueError("targets_on_device: labels must be (B,M,5|6) or (B,t,M,5|6) [x1, y1, x2, y2, id(, mix ratio)], got %r"
                         % (lab.shape,))
    M = lab.shape[-2]
    if M > MAX_GT:
        raise ValueError("targets_on_device: M=%d label rows per image, vd_yolo_targets takes at most %d" % (M, MAX_GT))
    flat = lab.reshape(-1, M, lab.shape[-1])
    valid = np.logical_and.accumulate((flat[..., :4] >= 0).all(axis=-1), axis=1)         # the host stops at the first padded row
    ids = flat[..., 4]
    bad = valid & ~((ids == np.floor(ids)) & (ids >= 0) & (ids < num_class))
    if bad.any():
        n, m = [int(v[0]) for v in np.nonzero(bad)]
        where = "sample %d" % n if lab.ndim == 3 else "sample %d frame %d" % divmod(n, lab.shape[1])
        raise ValueError("targets_on_device: %s, label row %d: class id %r is not an integer in [0, %d)"
                         % (where, m, float(ids[n, m]), num_class))
    return flat


def targets_on_device(labels, height, width, num_class):
    """The collated label batch of a `device_targets=True` loader -> (gt, obj, ctr, scl, wgt, cls) on the current device, fp32,
    with the shapes the host columns have: gt (B,M,4), the targets (B,P,1|2|2|2|C) - or (B,t,M,4) and (B,t,P,.) for per-frame
    labels.  One upload (the labels), one vd_yolo_targets call; the targets are `prefetch_targets`' (bit-equal but for the last
    bit of the scale targets' log).  There is no CPU fallback."""
    import torch
    from . import ops
    flat = check_labels(labels, num_class)
    lead, (N, M, w) = np.shape(labels)[:-2], flat.shape
    if not torch.cuda.is_available():
        raise RuntimeError("targets_on_device needs the GPU: the target kernel has no CPU fallback")
    Mk = max(M, 1)                                                                        # an all-empty batch: one padded row
    if M == 0:
        flat = np.full((N, 1, w), -1.0, np.float32)
    # gt, ids and mix as three contiguous sections of one buffer: one host-to-device copy
    parts = [flat[..., :4], flat[..., 4]] + ([flat[..., 5]] if w == 6 else [])
    dev = torch.from_numpy(np.concatenate([p.reshape(-1) for p in parts])).cuda()
    gt, ids = dev[:N * Mk * 4].view(N, Mk, 4), dev[N * Mk * 4:N * Mk * 5]
    mix = dev[N * Mk * 5:] if w == 6 else None
    P = num_rows(height, width)
    out = [torch.empty(lead + (P, c), dtype=torch.float32, device=dev.device) for c in (1, 2, 2, 2, num_class)]
    ops.yolo_targets(gt, ids, 1, mix, N, Mk, num_class, height, width, *out)
    return (gt[:, :M].reshape(lead + (M, 4)),) + tuple(out)
