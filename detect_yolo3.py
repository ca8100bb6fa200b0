#!/usr/bin/env python
"""Run YOLOv3 (Darknet-53) detection on MI355X — drop-in for the reference's detect_yolo3.py entry point.

Follows /root/reference/detect_yolo3.py: flags :41-118, detect() :198-272 (inference loop, clip, keep rows with
id >= 0, normalise boxes by W, collect [id, score, x1, y1, x2, y2] per image path), save_predictions :275-330
(one `path,id,score,x1,y1,x2,y2` text file per image), load_predictions/evaluate :333-448,659-695 (VOC mAP; the
reference's `sid=` keyword bug at :693 is not reproduced), main :792-939 (net build :871-892).
`--window K,1 --conv_types 21,...` detects with yolo3_3ddarknet (:872-882), the (2+1)-D Darknet backbone of frame windows.
The network underneath is viddet_amd.model.YOLOV3 (hand-written HIP kernels).  Frames shard across ranks with
no collective on the data path (inference = replicas only); the per-image box lists are gathered to rank 0, which writes
the prediction files and evaluates.  `--model_agnostic` (:797-798, :861-862, :893, :922-925) detects class-agnostically: one
candidate per anchor scored by its objectness, plain NMS over the image, predictions under pred_ag, results named *_ag.
`--metrics vid` scores the detections with the ImageNet VID motion metric (get_metric :188-190, evaluate :659-695, the result
files of :920-931; viddet_amd/vid_metric.py) on SyntheticTracks clips, `--device_metric` with the per-image matching on the
device (vd_vid_match).  `--metrics coco` (the default's second metric) scores them with the COCO detection metric
(get_metric :185-186; viddet_amd/coco_metric.py: the behaviour of the reference's wrapper and ground-truth JSON, COCOeval restated) and
writes coco.txt, `--device_metric` with the per-image matching on the device (vd_coco_match).  `--seq_nms` (no
reference counterpart) runs sequence NMS over the detections of every clip on the device (vd_seq_nms): the plain
predictions and results are written as without it, the rescored ones beside them under pred_seq and *_seq.  `--track` (no
reference counterpart) links the detections of every clip into tracks on the device (vd_track): every prediction
set gets a twin, pred_trk / pred_seq_trk, whose lines end in the row's track id, and tracks.txt / tracks_seq.txt count them per
clip; everything else is written as without the flag; `--track_method sort` links them with SORT instead (vd_track_sort, DESIGN.md
34; not with --live), `--track_method byte` with BYTE, SORT with a second association of the low-score rows (vd_track_byte,
DESIGN.md 36; not with --live); `--track_online` lifts both refusals: the live session then carries the SORT or BYTE tracker
itself from push to push (vd_track_kf_push).  `--live` (with --stream; no reference counterpart) sends every clip
through a live session (net.open_video) in pushes of --live_push frames and a flush, as a camera would hand it over:
the files and results are those of --stream byte for byte.  `--tubelet` (with --track; no reference counterpart) runs a tubelet
pass over every tracked clip on the device (vd_tubelet) - a track's rows take its score, the frames it skipped get
an interpolated box - and writes the rows after it beside everything else, under pred_tub, pred_tub_trk and *_tub.
`--track_smooth` (with --track; no reference counterpart) smooths the boxes of every tracked clip along its tracks on the device
(vd_track_smooth, DESIGN.md 37: the Rauch-Tung-Striebel smoother of SORT's Kalman filter) and writes the rows with their smoothed
boxes beside everything else, under pred_smo, pred_smo_trk and *_smo; not with --seq_nms or --tubelet, and with --live only
beside `--track_smooth_lag L`: the live session then smooths in fixed-lag form itself, every frame L frames late
(vd_track_smooth_push), and the same files are written with the session's boxes.  `--visualise [--display_gt]`
(with --stream; detect_yolo3.py visualise_predictions) draws what every clip's call returns - rings, tags of class, score and
track id, trails, the label rows in green underneath - onto the clip's frames on the device (vd_overlay) and writes
every --vis_every-th frame as vis/<clip>/<frame>.ppm; everything else is written as without the flag.
`--track_stitch` (with --track; no reference counterpart) re-links the track fragments of every tracked clip across gaps of up to
--track_stitch_gap frames on the device (vd_track_stitch) and writes the rows under their stitched ids beside
everything else, under pred_sti_trk, tracks_sti.txt and mot_sti.txt / hota_sti.txt - the detections do not change, so there is no
pred_sti; not with --live, --seq_nms, --tubelet or --track_smooth.  `--metrics mot`
(with --track; no reference counterpart) scores every tracked twin with the MOT tracking metric (viddet_amd/mot_metric.py: MOTA,
MOTP, id switches, fragmentations, IDF1, ... against the track ids of SyntheticTracks) on the rows read back from the
twin's files, and writes mot.txt / mot_seq.txt / mot_tub.txt; `--device_metric` with the per-frame matching on the device
(vd_mot_match).  `--metrics hota` (with --track; no reference counterpart) scores the same rows with the HOTA tracking metric
(viddet_amd/hota_metric.py: HOTA, DetA, AssA, LocA, ... over 19 localisation thresholds) and writes hota.txt /
hota_seq.txt / hota_tub.txt; `--device_metric` with the per-frame matching on the device (vd_hota_match).  Visualisation and the
worst-video tool are out of scope.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

from viddet_amd import dist as vdist
from viddet_amd.data import SyntheticDetection, SyntheticCombined, SyntheticPan, SyntheticTracks, SyntheticVideo, \
    YOLO3VideoInferenceTransform, Loader
from viddet_amd.metrics import VOCMApMetric
from viddet_amd.vid_metric import VIDDetectionMetric
from viddet_amd.coco_metric import COCODetectionMetric
from viddet_amd.hota_metric import HOTAMetric
from viddet_amd.mot_metric import MOTMetric
from viddet_amd.hierarchy import ClassTree, get_class_map, hierarchical_nms, iou  # noqa: F401  (detect_yolo3.py:698-789)
from viddet_amd.model import yolo3_darknet53, yolo3_3ddarknet, check_conv_types
from train_yolov3 import _list, _bool


def parse_flags(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    A = ap.add_argument
    A("--model_path", default="yolo3_darknet53_voc_best.params")
    A("--network", default="darknet53")
    A("--dataset", type=_list, default=["voc"])
    A("--trained_on", default="")
    A("--save_prefix", default="0001")
    A("--save_dir", default="results")
    A("--metrics", type=_list, default=["voc", "coco"])
    A("--batch_size", type=int, default=1)
    A("--data_shape", type=int, default=416)
    A("--detection_threshold", type=float, default=0.5)
    A("--max_do", type=int, default=-1)
    A("--every", type=float, default=25)
    A("--window", type=_list, default=["1", "1"])
    A("--k_join_type", default=None)
    A("--k_join_pos", default=None)
    A("--block_conv_type", default="2")
    A("--rnn_pos", default=None)
    A("--corr_pos", default=None)
    A("--corr_d", type=int, default=4)
    A("--motion_stream", default=None)
    A("--stream_gating", default=None)
    A("--conv_types", type=_list, default=["2"] * 6)
    A("--h_join_type", default=None)
    A("--hier", type=_list, default=["1"] * 5)
    A("--mult_out", type=_bool, nargs="?", const=True, default=False)
    A("--temp", type=_bool, nargs="?", const=True, default=False)
    A("--visualise", type=_bool, nargs="?", const=True, default=False)
    A("--per_frame_metric", type=_bool, nargs="?", const=True, default=False)
    A("--worst_video_path", default=None)
    A("--display_gt", type=_bool, nargs="?", const=True, default=True)
    A("--vis_thickness", type=int, default=None,
      help="(no reference counterpart) with --visualise: the pixels of a box outline and of a trail (default 2, as cv2.rectangle(.., 2))")
    A("--vis_scale", type=int, default=None, help="(no reference counterpart) with --visualise: the text scale, 1..4 (default 1)")
    A("--vis_trail", type=int, default=None,
      help="(no reference counterpart) with --visualise --track: the frames a track's trail reaches back, 0..16 (default 8)")
    A("--vis_every", type=int, default=None, help="(no reference counterpart) with --visualise: every n-th frame of a clip is written (default 1)")
    A("--model_agnostic", type=_bool, nargs="?", const=True, default=False)
    A("--metric_agnostic", type=_bool, nargs="?", const=True, default=False)
    A("--gpus", type=_list, default=["0"])
    A("--num_workers", type=int, default=8)
    A("--new_model", type=_bool, nargs="?", const=True, default=False)
    A("--offset", type=int, default=0)
    A("--hier_level", type=int, default=10)
    A("--synthetic_samples", type=int, default=32)
    A("--precision", default="fp32", choices=["fp32", "bf16"],
      help="(no reference counterpart) bf16: bf16 storage + bf16 MFMA inference, fp32 heads (net.set_precision, BASELINE configs[1])")
    A("--stream", type=_bool, nargs="?", const=True, default=False,
      help="(no reference counterpart) detect on whole synthetic clips with net.detect_video: the per-frame part of the network "
           "runs once per frame into a feature ring, --batch_size output frames per chunk; the same prediction files and metric "
           "as the windowed run on the same clips (DESIGN.md 19)")
    A("--device_resize", type=_bool, nargs="?", const=True, default=False,
      help="(no reference counterpart) ship the raw uint8 frames at their source size and resize them to --data_shape on the "
           "device, inside the kernel that normalises them (net.set_device_resize): the host's imresize leaves the per-frame "
           "path; predictions differ from the host-resized run only where the fp32 resample rounds a grey level the other "
           "way (DESIGN.md 20)")
    A("--frame_format", default="rgb", choices=["rgb", "nv12"],
      help="(no reference counterpart) nv12: the frames are NV12, as video decoders hand them out - a luma plane and a "
           "half-resolution plane of interleaved chroma pairs, (H0*3/2,W0) uint8 - and are converted to RGB inside the kernel "
           "that resizes them (net.set_device_resize(source='nv12')); needs --device_resize (DESIGN.md 23)")
    A("--yuv_matrix", default="bt601", choices=["bt601", "bt709"], help="the colour matrix of --frame_format nv12")
    A("--yuv_range", default="limited", choices=["limited", "full"], help="the range of --frame_format nv12")
    A("--synthetic_videos", type=int, default=None,
      help="(no reference counterpart) the dataset is SyntheticVideo: this many clips of --synthetic_samples frames each, "
           "windows by --window K,step inside a clip (default with --stream: 2; without --stream the windowed path runs on it)")
    A("--device_metric", type=_bool, nargs="?", const=True, default=False,
      help="(no reference counterpart) --metrics vid and --metrics coco match detections and ground truth on the GPU (vd_vid_match, "
           "vd_coco_match: one workgroup per image; DeviceVIDDetectionMetric, DeviceCOCODetectionMetric): the same vid.txt / "
           "coco.txt as the host metrics write (DESIGN.md 25, 26).  --metrics mot likewise (vd_mot_match: one workgroup per clip; "
           "DeviceMOTMetric): the same mot.txt (DESIGN.md 33).  --metrics hota likewise (vd_hota_match: a workgroup per frame; "
           "DeviceHOTAMetric): the same hota.txt (DESIGN.md 35)")
    A("--seq_nms", type=_bool, nargs="?", const=True, default=False,
      help="(no reference counterpart) sequence NMS (Han et al. 2016) over the detections of every clip, on the device "
           "(vd_seq_nms): boxes of adjacent frames are linked, the best sequence's rows take its score, what overlaps them is "
           "suppressed, until every row is decided.  Needs clips (--stream or --synthetic_videos).  The plain predictions and "
           "results are written as without the flag; the rescored ones go to pred_seq and *_seq files (DESIGN.md 27)")
    A("--seq_nms_link", type=float, default=0.5, help="--seq_nms: two boxes of adjacent frames link where their IoU exceeds this")
    A("--seq_nms_thresh", type=float, default=0.3, help="--seq_nms: a sequence's box suppresses the boxes of its frame whose IoU exceeds this")
    A("--seq_nms_rescore", default="avg", choices=["avg", "max"], help="--seq_nms: the score a sequence gives its boxes")
    A("--seq_nms_input_nms", type=float, default=0.45,
      help="--seq_nms: the nms_thresh of the per-frame NMS ahead of it (set_nms): higher lets more candidates through")
    A("--track", type=_bool, nargs="?", const=True, default=False,
      help="(no reference counterpart) link the detections of every clip into tracks on the device (vd_track): the IOU tracker of "
           "Bochinski et al. 2017 - a track takes the unclaimed box of its class with the largest IoU to its last box.  Needs clips "
           "(--stream or --synthetic_videos).  Every prediction set gets a twin (pred_trk, pred_seq_trk) whose lines end in the "
           "row's track id (-1: none), and tracks.txt / tracks_seq.txt hold `clip tracks rows mean_len` per clip; everything "
           "else is written as without the flag (DESIGN.md 28)")
    A("--live", type=_bool, nargs="?", const=True, default=False,
      help="(no reference counterpart) with --stream: every clip goes through a live session (net.open_video) in pushes of "
           "--live_push frames and a flush, as a camera or a decoder would hand it over; the prediction files and results are "
           "those of --stream byte for byte, --track included (its online ids are decided at the clip's end).  Not with "
           "--seq_nms, which has no online form")
    A("--live_push", type=int, default=1, help="--live: frames per push (default 1)")
    A("--track_method", default="iou", choices=["iou", "sort", "byte"],
      help="--track: iou (the default, vd_track), sort (vd_track_sort, DESIGN.md 34): SORT of Bewley et al. 2016 - every track is "
           "predicted by a constant-velocity Kalman filter and the predictions are matched to the frame's boxes by an optimal "
           "assignment, so a track survives missed frames of a moving object and crossing objects keep their ids - or byte "
           "(vd_track_byte, DESIGN.md 36): BYTE of Zhang et al. 2022 - SORT with two associations a frame: the boxes scored at "
           "least --track_det first, then the tracks left over against the lower-scored boxes, which never start a track, so a "
           "track survives a dip of its object's score and low-score clutter starts none.  The same files are written.  sort and "
           "byte: not with --live, unless --track_online is given")
    A("--track_online", type=_bool, nargs="?", const=True, default=False,
      help="(no reference counterpart) with --stream --live --track --track_method sort|byte: the live session carries that "
           "tracker from push to push on the device (net.open_video(track={..., 'online': True}), vd_track_kf_push, DESIGN.md "
           "39); the files and results are those of the --stream run byte for byte.  Not without --live and not with "
           "--track_method iou, whose tracker is always online")
    A("--track_app", type=_bool, nargs="?", const=True, default=False,
      help="(no reference counterpart) with --stream --track --track_method sort: appearance association (DESIGN.md 43) - every "
           "row gets an int8 descriptor pooled from the backbone's own route tensor under its box (vd_roi_embed) and SORT links on "
           "the fused cost of geometry and appearance (vd_track_sort_app): a box joins a track where its IoU to the predicted box "
           "is at least --track_iou, or at least --track_app_prox with a descriptor cosine of at least --track_app_cos.  The files "
           "are those --track_method sort writes.  Not with --live, --seq_nms, a late join or without --stream")
    A("--track_app_cos", type=float, default=None,
      help="--track_app: the least cosine of the descriptors of a box and a track that admits the pair, 0 to 1 (default 0.8, "
           "provisional)")
    A("--track_app_prox", type=float, default=None,
      help="--track_app: the least IoU to the predicted box at which appearance may admit a pair, 0 to 1 (default 0.1, provisional)")
    A("--track_app_level", type=int, default=None,
      help="--track_app: the stride of the route tensor the descriptors are pooled from, 8 (256 channels, the default), 16 or 32")
    A("--track_gmc", type=_bool, nargs="?", const=True, default=False,
      help="(no reference counterpart) with --stream --track: camera-motion compensation (DESIGN.md 44) - the translation of the "
           "whole picture between consecutive frames is estimated on the device from the frames' luma (vd_motion_sig, "
           "vd_motion_match), summed along the clip and taken off the boxes the tracker links (vd_motion_shift).  Every file of "
           "the run without the flag is written, from the same detections; motion.txt beside them holds one line `clip frame dx "
           "dy sad_best sad_zero` per frame.  Not with --live, --track_smooth, --tubelet or without --stream")
    A("--track_gmc_cell", type=int, default=None,
      help="--track_gmc: the side of a signature cell in source pixels, 2, 4, 8 or 16 (default 4): the unit of the motion")
    A("--track_gmc_radius", type=int, default=None,
      help="--track_gmc: the largest displacement searched per frame, in cells, 1 to 16 (default 8)")
    A("--track_gmc_gate", type=float, default=None,
      help="--track_gmc: the best displacement is taken where its SAD is at most this share of the SAD at no displacement, else "
           "the frame counts as unmoved; above 0, at most 1 (default 0.75, provisional)")
    A("--synthetic_pan", type=int, default=0,
      help="(no reference counterpart) the dataset is SyntheticPan: SyntheticTracks' objects seen by a camera that steps by up to "
           "this many pixels a frame over a textured canvas (default 0: the sets as before)")
    A("--track_iou", type=float, default=None,
      help="--track: a box joins a track where its IoU to the track's last box (sort, byte: its predicted box) is at least this "
           "(default: iou 0.5, sort 0.3, byte 0.2)")
    A("--track_low", type=float, default=None,
      help="--track: detections scored below this take no part (default: iou and sort 0.0, byte 0.1)")
    A("--track_det", type=float, default=None,
      help="--track_method byte: a detection scored at least this is a high-score box, matched first (default 0.5)")
    A("--track_new", type=float, default=None,
      help="--track_method byte: an unmatched high-score box starts a track where its score is at least this (default 0.6)")
    A("--track_iou2", type=float, default=None,
      help="--track_method byte: the IoU threshold of the second association, low-score boxes against the tracks left over (default 0.5)")
    A("--track_high", type=float, default=0.5, help="--track: a track is kept where its best score is at least this")
    A("--track_min_len", type=int, default=2, help="--track: a track is kept where it holds at least this many boxes")
    A("--track_max_age", type=int, default=None,
      help="--track: the frames in a row a track may go without a box before it is closed, 0 to 7 (default: iou 0, sort 1, "
           "the papers' values; byte 7)")
    A("--tubelet", type=_bool, nargs="?", const=True, default=False,
      help="(no reference counterpart) with --track: a tubelet pass over every tracked clip on the device (vd_tubelet): the rows "
           "of a track take the track's score, the frames a track skipped get a linearly interpolated box, every frame is "
           "re-sorted.  Everything a run without the flag writes is written unchanged; the rows after the pass go to pred_tub, "
           "their twin with track ids to pred_tub_trk, tracks_tub.txt and the --metrics files *_tub.txt (DESIGN.md 32).  Not with "
           "--live (a hole is known only after its frame was given out) and not with --seq_nms")
    A("--tubelet_rescore", default="avg", choices=["avg", "max", "none"], help="--tubelet: the score a track gives its rows (none: they keep theirs)")
    A("--tubelet_max_gap", type=int, default=7, help="--tubelet: holes of up to this many frames are filled, 0 (none) to 7")
    A("--tubelet_drop_untracked", type=_bool, nargs="?", const=True, default=False,
      help="--tubelet: the rows that no kept track holds are dropped")
    A("--track_smooth", type=_bool, nargs="?", const=True, default=False,
      help="(no reference counterpart) with --track: the boxes of every tracked clip are smoothed along its tracks on the device "
           "(vd_track_smooth): the Rauch-Tung-Striebel smoother of SORT's Kalman filter estimates every box of a track from the "
           "frames before and after it.  Everything a run without the flag writes is written unchanged; the smoothed rows go to "
           "pred_smo, their twin with track ids to pred_smo_trk, tracks_smo.txt and the --metrics files *_smo.txt (DESIGN.md 37).  "
           "Not with --live (a frame's smoothed box needs the frames after it) unless --track_smooth_lag is given, not with "
           "--seq_nms or --tubelet")
    A("--track_smooth_gap", type=int, default=7,
      help="--track_smooth: a track is cut where it skips more than this many frames, 0 to 7")
    A("--track_smooth_lag", type=int, default=None,
      help="(no reference counterpart) with --stream --live --track --track_smooth: the live session smooths the boxes itself in "
           "fixed-lag form (net.open_video(smooth={'lag': L}), vd_track_smooth_push, DESIGN.md 40): every frame comes out this "
           "many frames late, 0 to 15, its boxes estimated from the frames before it and that many after it.  It lifts the "
           "refusal of --track_smooth beside --live; the files are those of the --stream --track --track_smooth run, with the "
           "session's boxes.  Not without --live and not without --track_smooth")
    A("--track_stitch", type=_bool, nargs="?", const=True, default=False,
      help="(no reference counterpart) with --track: the track fragments of every tracked clip are re-linked across long gaps on "
           "the device (vd_track_stitch): a track's filter state at its last row is extrapolated over the gap and matched to the "
           "first rows of later tracks, and every chain takes its first fragment's id.  Everything a run without the flag writes "
           "is written unchanged; the rows under their stitched ids go to pred_sti_trk, tracks_sti.txt and the --metrics files "
           "mot_sti.txt / hota_sti.txt (DESIGN.md 38).  Not with --live (a fragment's successor is known only later), --seq_nms, "
           "--tubelet or --track_smooth")
    A("--track_stitch_gap", type=int, default=None,
      help="--track_stitch: a tail is extrapolated over at most this many frames, 1 to 32 (default 30)")
    A("--track_stitch_iou", type=float, default=None,
      help="--track_stitch: the least IoU of an extrapolated tail and a head (default 0.3)")
    A("--synthetic_classes", type=int, default=None, help="classes per dataset of the synthetic combined set (default: the datasets' own counts)")
    A("--random_init", type=_bool, nargs="?", const=True, default=False,
      help="skip load_parameters (no checkpoint available offline)")
    FLAGS = ap.parse_args(argv)
    # --track_iou / --track_max_age / --track_low left out: the linking method's own defaults (iou: 0.5, 0 and 0.0, sort: 0.3, 1
    # and 0.0, byte: 0.2, 7 and 0.1); byte's own three flags stay None beside another method, where check_flags refuses them
    track_defaults = _track_defaults(FLAGS.track_method)
    for flag, key in (("track_iou", "sigma_iou"), ("track_max_age", "max_age"), ("track_low", "sigma_l")) + _BYTE_FLAGS:
        if getattr(FLAGS, flag) is None and key in track_defaults:
            setattr(FLAGS, flag, track_defaults[key])
    return FLAGS


_BYTE_FLAGS = (("track_det", "sigma_d"), ("track_new", "sigma_new"), ("track_iou2", "sigma_iou2"))   # --track_method byte's own


def _track_defaults(method):
    """the DEFAULTS of a --track_method"""
    if method == "sort":
        from viddet_amd.sort import DEFAULTS
    elif method == "byte":
        from viddet_amd.byte import DEFAULTS
    else:
        from viddet_amd.track import DEFAULTS
    return DEFAULTS


def _collect(boxes, dataset, ids, scores, bboxes, sidxs, W):
    """detect_yolo3.py:228-262: clip, keep rows with a class, normalise the boxes, file them under the image path"""
    ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
    bboxes = np.clip(bboxes.cpu().numpy(), 0, W)                           # :228 clip to image size
    for id_, score, box, sidx in zip(ids, scores, bboxes, sidxs):
        file = dataset.sample_path(int(sidx))
        valid = np.where(id_.flat >= 0)[0]                                 # :255 boxes that have a class
        box = box[valid, :] / W                                            # :257 normalise boxes
        for i_, b_, s_ in zip(id_.flat[valid].astype(int), box, score.flat[valid]):
            boxes.setdefault(file, []).append([i_, s_] + list(b_))


def seq_nms_args(FLAGS):
    """the dict net.detect_video and ops.seq_nms take, None without --seq_nms"""
    if not getattr(FLAGS, "seq_nms", False):
        return None
    return dict(link_thresh=FLAGS.seq_nms_link, nms_thresh=FLAGS.seq_nms_thresh, rescore=FLAGS.seq_nms_rescore)


def track_args(FLAGS):
    """the dict net.detect_video and link_rows take, None without --track: ops.track's parameters and, with --track_method
    sort or byte, `method` (byte: sigma_d, sigma_new and sigma_iou2 too); --track_iou, --track_max_age and --track_low left out
    take the method's defaults (iou: 0.5, 0 and 0.0, sort: 0.3, 1 and 0.0, byte: 0.2, 7 and 0.1)"""
    if not getattr(FLAGS, "track", False):
        return None
    method = getattr(FLAGS, "track_method", "iou")
    DEFAULTS = _track_defaults(method)

    def given(flag, key):
        v = getattr(FLAGS, flag, None)
        return DEFAULTS[key] if v is None else v

    args = dict(sigma_iou=given("track_iou", "sigma_iou"), sigma_l=given("track_low", "sigma_l"), sigma_h=FLAGS.track_high,
                t_min=FLAGS.track_min_len, max_age=given("track_max_age", "max_age"))
    if method == "byte":
        args.update({key: given(flag, key) for flag, key in _BYTE_FLAGS})
    if getattr(FLAGS, "track_app", False):
        args["appearance"] = app_args(FLAGS)
    if getattr(FLAGS, "track_gmc", False):
        args["gmc"] = gmc_args(FLAGS)
    return dict(args, method=method) if method != "iou" else args


_GMC_FLAGS = (("track_gmc_cell", "cell"), ("track_gmc_radius", "radius"), ("track_gmc_gate", "gate"))           # --track_gmc's own


def gmc_args(FLAGS):
    """the `gmc` dict of detect_video's track option, None without --track_gmc; a flag left out takes viddet_amd.motion's
    default"""
    if not getattr(FLAGS, "track_gmc", False):
        return None
    from viddet_amd.motion import DEFAULTS
    return {key: DEFAULTS[key] if getattr(FLAGS, flag, None) is None else getattr(FLAGS, flag) for flag, key in _GMC_FLAGS}


_APP_FLAGS = (("track_app_cos", "sigma_app"), ("track_app_prox", "sigma_prox"), ("track_app_level", "level"))   # --track_app's own


def app_args(FLAGS):
    """the `appearance` dict of detect_video's track option, None without --track_app; a flag left out takes
    viddet_amd.appearance's default"""
    if not getattr(FLAGS, "track_app", False):
        return None
    from viddet_amd.appearance import OPTION_DEFAULTS
    return {key: OPTION_DEFAULTS[key] if getattr(FLAGS, flag, None) is None else getattr(FLAGS, flag) for flag, key in _APP_FLAGS}


def link_rows(ids, scores, bboxes, track, **kw):
    """the track id of every row: ops.track, or with track_args' method 'sort' ops.track_sort and with 'byte' ops.track_byte, on
    the rows of whole clips"""
    from viddet_amd import ops
    track = dict(track)
    link = dict(iou=ops.track, sort=ops.track_sort, byte=ops.track_byte)[track.pop("method", "iou")]
    return link(ids, scores, bboxes, **kw, **track)[0]


def tubelet_args(FLAGS):
    """the dict net.detect_video and ops.tubelet take, None without --tubelet"""
    if not getattr(FLAGS, "tubelet", False):
        return None
    return dict(rescore=None if FLAGS.tubelet_rescore == "none" else FLAGS.tubelet_rescore, max_gap=FLAGS.tubelet_max_gap,
                drop_untracked=FLAGS.tubelet_drop_untracked)


def smooth_args(FLAGS):
    """the dict net.detect_video and ops.smooth take, None without --track_smooth"""
    if not getattr(FLAGS, "track_smooth", False):
        return None
    return dict(max_gap=FLAGS.track_smooth_gap)


def _collect_tracks(tracks, dataset, ids, track, sidxs):
    """the track id of every row _collect files, in its order, under the same image path"""
    ids, track = ids.cpu().numpy(), track.cpu().numpy()
    for id_, tr, sidx in zip(ids, track, sidxs):
        valid = np.where(id_.flat >= 0)[0]
        tracks.setdefault(dataset.sample_path(int(sidx)), []).extend(int(v) for v in tr[valid])


def clip_offsets(sidxs, frames_per_video):
    """sample indices in ascending order -> the offsets at which a clip starts (and the end): a clip is a run of consecutive
    frames of one video"""
    cs = [0]
    for n in range(1, len(sidxs)):
        if sidxs[n] != sidxs[n - 1] + 1 or sidxs[n] // frames_per_video != sidxs[n - 1] // frames_per_video:
            cs.append(n)
    return cs + [len(sidxs)]


def stitch_args(FLAGS):
    """the dict net.detect_video and ops.stitch take, None without --track_stitch"""
    if not getattr(FLAGS, "track_stitch", False):
        return None
    gap, iou = getattr(FLAGS, "track_stitch_gap", None), getattr(FLAGS, "track_stitch_iou", None)
    return dict(max_gap=30 if gap is None else gap, sigma_iou=0.3 if iou is None else iou)


def detect(net, dataset, loader, max_do=-1, data_shape=None, seq_nms=None, input_nms=0.45, track=None, tubelet=None, smooth=None,
           stitch=None):
    """detect_yolo3.py:198-272.  data_shape: the size the network detects at where the loader's frames are not that size
    (--device_resize: raw frames, resized on the device).  seq_nms (a dict of link_thresh / nms_thresh / rescore): every
    batch's outputs stay on the device, and ONE ops.seq_nms call over all clips follows the loop; returns (boxes, rescored).
    track (a dict of ops.track's parameters): the outputs stay on the device likewise and ONE ops.track call per prediction set
    follows; returns (boxes, rescored or None, tracks, tracks of the rescored or None).  tubelet (a dict of ops.tubelet's
    parameters, with track and without seq_nms): ONE ops.tubelet call over all tracked clips follows; the rows after the pass
    and their track ids are returned as a fifth and a sixth element.  smooth (a dict of ops.smooth's parameter, with track and
    without seq_nms and tubelet): ONE ops.smooth call over all tracked clips follows; the rows with their smoothed boxes and
    their track ids are returned as that fifth and sixth element.  stitch (a dict of ops.stitch's parameters, with track and
    without the three): ONE ops.stitch call over all tracked clips follows; the fifth element is None - the rows are the plain
    ones - and the sixth holds their stitched ids."""
    net.set_nms(nms_thresh=input_nms, nms_topk=400)
    boxes = dict()
    if max_do < 0:
        max_do = len(dataset)
    c = 0
    kept, W = [], None
    for x, _label, sidxs in loader:
        ids, scores, bboxes = net(torch.from_numpy(x).cuda())
        W = data_shape or (x.shape[-2] if x.dtype == np.uint8 else x.shape[-1])   # uint8 frames are (B,H,W,3)
        if seq_nms is None and track is None:
            _collect(boxes, dataset, ids, scores, bboxes, sidxs, W)
        else:                                                              # the plan's output tensors are rewritten by the next batch
            kept.append((ids.clone(), scores.clone(), bboxes.clone(), [int(i) for i in sidxs]))
        c += x.shape[0]
        if c > max_do:
            break
    if seq_nms is None and track is None:
        return boxes
    from viddet_amd import ops
    boxes_seq = dict()
    tracks, tracks_seq = dict(), dict()
    boxes_tub, tracks_tub = dict(), dict()
    if kept:
        sidxs = [i for k in kept for i in k[3]]
        order = sorted(range(len(sidxs)), key=lambda n: sidxs[n])          # clip order: sample = video * frames + frame
        sidxs = [sidxs[n] for n in order]
        gather = torch.tensor(order, device=kept[0][0].device)
        ids, scores, bboxes = [torch.cat([k[a] for k in kept])[gather].contiguous() for a in range(3)]
        if ids.shape[1] > 128:
            raise ValueError("%s: post_nms=%d rows per frame, %s at most 128"
                             % (("--track", ids.shape[1], "the tracker takes") if seq_nms is None else
                                ("--seq_nms", ids.shape[1], "Seq-NMS takes")))
        bboxes = bboxes.clamp(0, W)                                        # Seq-NMS and the tracker see the boxes as they are saved (:228)
        cs = clip_offsets(sidxs, dataset.frames_per_video)
        C = 1 if net.agnostic else net.num_class
        _collect(boxes, dataset, ids, scores, bboxes, sidxs, W)
        if track is not None:
            linked = link_rows(ids, scores, bboxes, track, clip_start=cs, num_class=C)
            _collect_tracks(tracks, dataset, ids, linked, sidxs)
            if tubelet is not None:
                out = ops.tubelet(ids, scores, bboxes, linked, clip_start=cs, num_class=C, **tubelet)
                _collect(boxes_tub, dataset, out[0], out[1], out[2], sidxs, W)
                _collect_tracks(tracks_tub, dataset, out[0], out[4], sidxs)
            elif smooth is not None:
                sbox, _ = ops.smooth(ids, scores, bboxes, linked, clip_start=cs, num_class=C, **smooth)
                _collect(boxes_tub, dataset, ids, scores, sbox, sidxs, W)
                _collect_tracks(tracks_tub, dataset, ids, linked, sidxs)
            elif stitch is not None:
                _collect_tracks(tracks_tub, dataset, ids, ops.stitch(ids, scores, bboxes, linked, clip_start=cs, num_class=C, **stitch)[0],
                                sidxs)
        if seq_nms is not None:
            out = ops.seq_nms(ids, scores, bboxes, clip_start=cs, num_class=C, **seq_nms)
            _collect(boxes_seq, dataset, out[0], out[1], out[2], sidxs, W)
            if track is not None:
                _collect_tracks(tracks_seq, dataset, out[0], link_rows(out[0], out[1], out[2], track, clip_start=cs, num_class=C), sidxs)
    if track is None:
        return boxes, boxes_seq
    if tubelet is not None or smooth is not None:
        return boxes, None, tracks, None, boxes_tub, tracks_tub
    if stitch is not None:
        return boxes, None, tracks, None, None, tracks_tub
    return (boxes, boxes_seq, tracks, tracks_seq) if seq_nms is not None else (boxes, None, tracks, None)


def live_clip(net, frames, step, chunk, push, track=None, smooth=None):
    """--live: detect_video(frames, step, chunk, track) by way of a live session - pushes of `push` frames, then a flush ->
    (ids, scores, bboxes, the (track, tlen, tscore) of detect_video's last_tracks or None).  The session's online tracker
    decides nothing; finalize_tracks decides at the clip's end, from the rows the session gave out.  Where the session keeps
    the filtered boxes of its rows (track with 'method': 'sort' or 'byte' and 'online': True), they are collected too and a
    fourth array, detect_video's last_track_boxes, ends the tuple.  smooth (open_video's dict, with 'lag'): the
    session smooths the boxes along the online tracker's tracks and gives every frame out 'lag' frames late; the boxes
    returned are the smoothed ones, and a fifth element holds the boxes ahead of the pass (session.last_pre_smooth)."""
    session = net.open_video(step=step, chunk=chunk, track=track, **({} if smooth is None else dict(smooth=smooth)))
    outs, trks, tboxes, pres = [], [], [], []
    for a in range(0, frames.shape[0], push):
        outs.append(session.push(frames[a:a + push])[1:])
        trks.append(session.last_tracks)
        tboxes.append(session.last_track_boxes)
        pres.append(session.last_pre_smooth)
    outs.append(session.flush()[1:])
    trks.append(session.last_tracks)
    tboxes.append(session.last_track_boxes)
    pres.append(session.last_pre_smooth)
    ids, scores, bboxes = (torch.cat(t) for t in zip(*outs))
    assert ids.shape[0] == frames.shape[0], "the session gave out %d of %d frames" % (ids.shape[0], frames.shape[0])
    if track is None:
        return ids, scores, bboxes, None
    from viddet_amd.track import finalize_tracks
    online = [torch.cat(t).cpu().numpy() for t in zip(*trks)]
    tbox = None if tboxes[0] is None else torch.cat(tboxes).cpu().numpy()
    final = finalize_tracks(*online, tbox=tbox, **session.track_decide)
    if smooth is not None:
        return ids, scores, bboxes, tuple(torch.from_numpy(a) for a in final), torch.cat(pres)
    return ids, scores, bboxes, tuple(torch.from_numpy(a) for a in final)


def detect_stream(net, dataset, data_shape, step, chunk, max_do=-1, rank=0, world=1, device_resize=False, frame_format="rgb",
                  seq_nms=None, input_nms=0.45, track=None, live=None, tubelet=None, smooth=None, stitch=None, track_online=False,
                  smooth_lag=None, visualise=None, motion_log=None):
    """--stream: what detect() collects, one whole clip at a time through net.detect_video - whole clips are sharded over
    the ranks (a clip's feature ring lives on one GPU).  device_resize: the clip travels at its source size (frame_format
    'nv12': as NV12 frames).  seq_nms (a dict): handed to detect_video; returns (boxes, rescored), the plain rows being the
    ones detect_video keeps in net.last_plain.  track (a dict): handed to detect_video too, which links the rows it returns;
    the plain rows ahead of Seq-NMS are linked by a call of their own; returns (boxes, rescored or None, tracks, tracks of the
    rescored or None).  live (--live_push, a number of frames): every clip goes through live_clip instead, with track_online
    (--track_online) on a session that carries the SORT or BYTE tracker of `track` itself.  tubelet (a dict,
    with track, without seq_nms and live): handed to detect_video as well; the plain rows are the ones it keeps in
    net.last_pre_tubelet, and the rows after the pass and their track ids are returned as a fifth and a sixth element.  smooth
    (a dict, with track, without seq_nms, live and tubelet): handed to detect_video likewise; the plain boxes are the ones it
    keeps in net.last_pre_smooth, and the rows with their smoothed boxes and their track ids are that fifth and sixth element;
    with live and smooth_lag (--track_smooth_lag) the live session smooths in fixed-lag form itself and the same
    six elements come from its rows, the track ids finalize_tracks' as ever.
    stitch (a dict, with track, without the four): handed to detect_video likewise; the tracker's ids are the ones it keeps in
    net.last_pre_stitch, the fifth element is None and the sixth holds the stitched ids of the plain rows.
    visualise (visualise_args' dict, not with live): detect_video draws what it returns onto every clip's frames on the device
    (its `overlay`) and write_overlay writes every `every`-th one as a PPM file; nothing else changes.
    motion_log (a list, with a `gmc` key in track: --track_gmc): receives (clip, frame, dx, dy, sad_best, sad_zero)
    for every frame, from net.last_motion."""
    net.set_nms(nms_thresh=input_nms, nms_topk=400)
    tf = YOLO3VideoInferenceTransform(data_shape, data_shape, device_normalize=True, device_resize=device_resize,
                                      frame_format=frame_format)
    boxes, boxes_seq = dict(), dict()
    tracks, tracks_seq = dict(), dict()
    boxes_tub, tracks_tub = dict(), dict()
    if max_do < 0:
        max_do = len(dataset)
    c = 0
    for v in range(rank, dataset.num_videos, world):
        x, _, _ = tf(dataset.video_frames(v), np.zeros((0, 6)))            # uint8 (T,H,W,3), normalised on the device
        sidxs = [dataset.sample_index(v, t) for t in range(x.shape[0])]
        W = data_shape if device_resize else x.shape[-2]
        trk_kw = {} if track is None else dict(track=dict(track, clip=W))  # the tracker sees the boxes as they are saved too
        if visualise is not None:
            trk_kw = dict(trk_kw, overlay=dict(visualise["params"], gt=clip_labels(dataset, sidxs, data_shape)
                                               if visualise["display_gt"] else None))
        if live is not None:
            live_trk = trk_kw.get("track")
            if track_online and live_trk is not None:                      # the session carries the method's own tracker
                live_trk = dict(live_trk, online=True)
            if smooth is not None:                                         # the session's own fixed-lag smoother
                ids, scores, sbox, last, bboxes = live_clip(net, torch.from_numpy(x), step, chunk, live, live_trk,
                                                            dict(smooth, lag=smooth_lag))
                _collect(boxes_tub, dataset, ids, scores, sbox, sidxs, W)
                _collect_tracks(tracks_tub, dataset, ids, last[0], sidxs)
            else:
                ids, scores, bboxes, last = live_clip(net, torch.from_numpy(x), step, chunk, live, live_trk)
            if track is not None:
                _collect_tracks(tracks, dataset, ids, last[0], sidxs)
        elif tubelet is not None:
            out = net.detect_video(torch.from_numpy(x), step=step, chunk=chunk, tubelet=tubelet, **trk_kw)
            _collect(boxes_tub, dataset, out[0], out[1], out[2], sidxs, W)
            _collect_tracks(tracks_tub, dataset, out[0], net.last_tubelet[1], sidxs)
            ids, scores, bboxes = net.last_pre_tubelet                     # the plain rows, clipped as _collect clips them
            _collect_tracks(tracks, dataset, ids, net.last_tracks[0], sidxs)
        elif smooth is not None:
            ids, scores, sbox = net.detect_video(torch.from_numpy(x), step=step, chunk=chunk, smooth=smooth, **trk_kw)
            _collect(boxes_tub, dataset, ids, scores, sbox, sidxs, W)
            _collect_tracks(tracks_tub, dataset, ids, net.last_tracks[0], sidxs)
            bboxes = net.last_pre_smooth                                   # the plain boxes, clipped as _collect clips them
            _collect_tracks(tracks, dataset, ids, net.last_tracks[0], sidxs)
        elif stitch is not None:
            ids, scores, bboxes = net.detect_video(torch.from_numpy(x), step=step, chunk=chunk, stitch=stitch, **trk_kw)
            _collect_tracks(tracks, dataset, ids, net.last_pre_stitch[0], sidxs)
            _collect_tracks(tracks_tub, dataset, ids, net.last_tracks[0], sidxs)
        elif seq_nms is None:
            ids, scores, bboxes = net.detect_video(torch.from_numpy(x), step=step, chunk=chunk, **trk_kw)
            if track is not None:
                _collect_tracks(tracks, dataset, ids, net.last_tracks[0], sidxs)
        else:
            # Seq-NMS sees the boxes as they are saved: clipped to the image (:228)
            out = net.detect_video(torch.from_numpy(x), step=step, chunk=chunk, seq_nms=dict(seq_nms, clip=W), **trk_kw)
            _collect(boxes_seq, dataset, out[0], out[1], out[2], sidxs, W)
            ids, scores, bboxes = net.last_plain
            if track is not None:
                from viddet_amd import ops
                _collect_tracks(tracks_seq, dataset, out[0], net.last_tracks[0], sidxs)
                plain = link_rows(ids, scores, bboxes.clamp(0, W), track, num_class=1 if net.agnostic else net.num_class)
                _collect_tracks(tracks, dataset, ids, plain, sidxs)
        _collect(boxes, dataset, ids, scores, bboxes, sidxs, W)
        if motion_log is not None and net.last_motion is not None:
            motion, sad = (t.cpu().tolist() for t in net.last_motion)
            motion_log.extend((v, t, m[0], m[1], s[0], s[1]) for t, (m, s) in enumerate(zip(motion, sad)))
        if visualise is not None:
            write_overlay(visualise, v, net.last_overlay[0])
        c += x.shape[0]
        if c > max_do:
            break
    if tubelet is not None or smooth is not None:
        return boxes, None, tracks, None, boxes_tub, tracks_tub
    if stitch is not None:
        return boxes, None, tracks, None, None, tracks_tub
    if track is not None:
        return (boxes, boxes_seq, tracks, tracks_seq) if seq_nms is not None else (boxes, None, tracks, None)
    return boxes if seq_nms is None else (boxes, boxes_seq)


def visualise_args(FLAGS, dataset=None):
    """--visualise: the dict detect_stream takes, None without the flag - `params` for detect_video's overlay (rows are drawn
    from --detection_threshold on, as the reference's visualise_predictions does, detect_yolo3.py:561; class names cut
    to the 15 characters a tag holds), `dir` <save_dir>/<save_prefix>/vis, `every`, `display_gt`, `yuv` (matrix, range) where
    the frames are NV12"""
    if not getattr(FLAGS, "visualise", False):
        return None
    params = dict(thresh=float(FLAGS.detection_threshold), thickness=2 if FLAGS.vis_thickness is None else FLAGS.vis_thickness,
                  scale=1 if FLAGS.vis_scale is None else FLAGS.vis_scale, trail=8 if FLAGS.vis_trail is None else FLAGS.vis_trail)
    if dataset is not None and not FLAGS.model_agnostic:
        params["class_names"] = tuple("".join(ch if 32 <= ord(ch) <= 126 else "?" for ch in str(n))[:15] for n in dataset.classes)
    return dict(params=params, dir=os.path.join(FLAGS.save_dir, FLAGS.save_prefix, "vis"),
                every=1 if FLAGS.vis_every is None else FLAGS.vis_every, display_gt=bool(FLAGS.display_gt),
                yuv=(FLAGS.yuv_matrix, FLAGS.yuv_range) if FLAGS.frame_format == "nv12" else None)


def clip_labels(dataset, sidxs, data_shape):
    """--display_gt: the label rows of a clip's frames as detect_video's overlay takes them - (T,G,5) float32 x1, y1, x2, y2,
    class in the predictions' coordinates (the data_shape square), padded with rows of -1"""
    w0, h0 = dataset.frame_size
    rows = [np.asarray(dataset[int(i)][1], np.float64).reshape(-1, 6)[:128] for i in sidxs]
    gt = np.full((len(rows), max(1, max(len(r) for r in rows)), 5), -1.0, np.float32)
    for t, r in enumerate(rows):
        gt[t, :len(r), :4] = r[:, :4] * (data_shape / w0, data_shape / h0, data_shape / w0, data_shape / h0)
        gt[t, :len(r), 4] = r[:, 4]
    return gt


def write_overlay(visualise, v, frames):
    """--visualise: every `every`-th painted frame of clip v as binary PPM vis/<clip %04d>/<frame %06d>.ppm; NV12 frames
    are converted on the host (video.nv12_to_rgb) first"""
    out = os.path.join(visualise["dir"], "%04d" % v)
    os.makedirs(out, exist_ok=True)
    every = visualise["every"]
    picked = frames[::every].cpu().numpy()
    if visualise["yuv"] is not None:
        from viddet_amd.video import nv12_to_rgb
        picked = nv12_to_rgb(np.ascontiguousarray(picked), *visualise["yuv"])
    for k, img in enumerate(picked):
        with open(os.path.join(out, "%06d.ppm" % (k * every)), "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
            f.write(np.ascontiguousarray(img).tobytes())


def pred_dir(save_dir, save_prefix, agnostic=False, seq=False, trk=False, tub=False):
    """detect_yolo3.py:275-279, 333-337: predictions of an agnostic model live beside the per-class ones, under pred_ag;
    seq: the predictions rescored by --seq_nms, under pred_seq / pred_ag_seq; trk: the twin of either whose lines end in the
    track id of --track, `_trk` last; tub: the rows after the pass of --tubelet, under pred_tub / pred_ag_tub ('smo': those of
    --track_smooth, under pred_smo / pred_ag_smo; 'sti': the twin under the stitched ids of --track_stitch, pred_sti_trk)"""
    return os.path.join(save_dir, save_prefix, ("pred_ag" if agnostic else "pred") + ("_seq" if seq else "") + _pass_tail(tub)
                        + ("_trk" if trk else ""))


def _pass_tail(tub):
    """what the files of the rows after a pass over the tracks carry in their names: True (--tubelet) _tub, 'smo'
    (--track_smooth) _smo, 'sti' (--track_stitch) _sti, False nothing"""
    return "_tub" if tub is True else "_" + tub if tub else ""


def result_name(metric_name, model_agnostic=False, metric_agnostic=False, seq=False, tub=False):
    """detect_yolo3.py:920-925 (--model_agnostic sets --metric_agnostic, :797-798; `_met` marks a class-agnostic metric over a
    per-class model, which only the vid metric has); seq: the metric of the predictions rescored by --seq_nms, `_seq` last; tub:
    the metric of the rows after the pass of --tubelet, `_tub` last ('smo': of --track_smooth, `_smo`)"""
    tail = ("_seq" if seq else "") + _pass_tail(tub)
    if model_agnostic:
        return metric_name + "_ag" + tail
    return (metric_name + "_ag_met" if metric_agnostic else metric_name) + tail


def check_flags(FLAGS):
    """What the parsed flags ask for that is not built is refused here, before anything touches the GPU; returns the checked
    conv_types (None: the plain 2-D backbone)."""
    mot = "mot" in [m.lower() for m in (getattr(FLAGS, "metrics", None) or [])]
    if mot:
        # the MOT metric scores tracks against the ground-truth tracks of a clip
        if not getattr(FLAGS, "track", False):
            raise NotImplementedError("--metrics mot needs --track: it scores the tracks of the tracked prediction sets (pred_trk, ...)")
        if len(FLAGS.dataset) > 1:
            raise NotImplementedError("--metrics mot does not combine with several --dataset names: the combined set has no "
                                      "clips and no ground-truth tracks")
        if getattr(FLAGS, "mult_out", False):
            raise NotImplementedError("--metrics mot does not combine with --mult_out: its rows are not the detections of one frame")
    hota = "hota" in [m.lower() for m in (getattr(FLAGS, "metrics", None) or [])]
    if hota:
        # the HOTA metric scores the same tracks against the same ground-truth tracks: refused where mot is
        if not getattr(FLAGS, "track", False):
            raise NotImplementedError("--metrics hota needs --track: it scores the tracks of the tracked prediction sets (pred_trk, ...)")
        if len(FLAGS.dataset) > 1:
            raise NotImplementedError("--metrics hota does not combine with several --dataset names: the combined set has no "
                                      "clips and no ground-truth tracks")
        if getattr(FLAGS, "mult_out", False):
            raise NotImplementedError("--metrics hota does not combine with --mult_out: its rows are not the detections of one frame")
    if getattr(FLAGS, "seq_nms", False):
        # Seq-NMS links the frames of a clip: a set without clips has nothing to link
        if len(FLAGS.dataset) > 1:
            raise NotImplementedError("--seq_nms does not combine with several --dataset names: the combined set has no clips")
        if getattr(FLAGS, "mult_out", False):
            raise NotImplementedError("--seq_nms does not combine with --mult_out: its rows are not the detections of one frame")
        if not getattr(FLAGS, "stream", False) and getattr(FLAGS, "synthetic_videos", None) is None:
            raise NotImplementedError("--seq_nms needs clips: give --stream or --synthetic_videos (the plain synthetic set is "
                                      "unrelated still images)")
        if getattr(FLAGS, "seq_nms_rescore", "avg") not in ("avg", "max"):
            raise NotImplementedError("--seq_nms_rescore must be avg or max, got %r" % (FLAGS.seq_nms_rescore,))
        if not 0 < getattr(FLAGS, "seq_nms_input_nms", 0.45) < 1:
            raise NotImplementedError("--seq_nms_input_nms must lie inside (0, 1), got %r" % (FLAGS.seq_nms_input_nms,))
    if getattr(FLAGS, "live", False):
        # a live session is detect_video on a clip that arrives in pieces
        if not getattr(FLAGS, "stream", False):
            raise NotImplementedError("--live needs --stream: a live session is the streaming path (net.detect_video) on a clip "
                                      "that arrives in pieces; the windowed path has no clips to push")
        if getattr(FLAGS, "seq_nms", False):
            raise NotImplementedError("--live does not combine with --seq_nms: Seq-NMS revisits every frame of a clip until no "
                                      "row is alive, so no frame is final before the clip ends - it has no online form")
        if isinstance(getattr(FLAGS, "live_push", 1), bool) or int(getattr(FLAGS, "live_push", 1)) < 1:
            raise NotImplementedError("--live_push must be at least 1 (the frames per push), got %r" % (FLAGS.live_push,))
    if getattr(FLAGS, "track", False):
        # the tracker links the frames of a clip: refused where --seq_nms is, for its reasons
        if len(FLAGS.dataset) > 1:
            raise NotImplementedError("--track does not combine with several --dataset names: the combined set has no clips")
        if getattr(FLAGS, "mult_out", False):
            raise NotImplementedError("--track does not combine with --mult_out: its rows are not the detections of one frame")
        if not getattr(FLAGS, "stream", False) and getattr(FLAGS, "synthetic_videos", None) is None:
            raise NotImplementedError("--track needs clips: give --stream or --synthetic_videos (the plain synthetic set is "
                                      "unrelated still images)")
        if getattr(FLAGS, "track_method", "iou") not in ("iou", "sort", "byte"):
            raise NotImplementedError("--track_method must be iou, sort or byte, got %r" % (FLAGS.track_method,))
        for flag, _ in _BYTE_FLAGS:
            if getattr(FLAGS, "track_method", "iou") != "byte" and getattr(FLAGS, flag, None) is not None:
                raise NotImplementedError("--%s belongs to --track_method byte: --track_method %s has no such threshold"
                                          % (flag, getattr(FLAGS, "track_method", "iou")))
        if getattr(FLAGS, "track_method", "iou") != "iou" and getattr(FLAGS, "live", False) and not getattr(FLAGS, "track_online", False):
            raise NotImplementedError("--track_method %s does not combine with --live: it has no resumable form yet, a live "
                                      "session carries the iou tracker only" % FLAGS.track_method)
        if getattr(FLAGS, "track_online", False):
            # the resumable form of sort and byte is a live session's: refused elsewhere, never ignored
            if not getattr(FLAGS, "live", False):
                raise NotImplementedError("--track_online needs --live: it makes the live session (net.open_video) carry the "
                                          "--track_method's tracker; without --live every clip is tracked at its end")
            if getattr(FLAGS, "track_method", "iou") == "iou":
                raise NotImplementedError("--track_online does not combine with --track_method iou: that tracker is always "
                                          "online in a live session; the flag belongs to --track_method sort and byte")
        from viddet_amd.byte import check_byte_params
        from viddet_amd.track import check_params
        try:
            params = {k: v for k, v in track_args(FLAGS).items() if k not in ("method", "appearance", "gmc")}
            (check_byte_params if getattr(FLAGS, "track_method", "iou") == "byte" else check_params)(who="--track", **params)
        except ValueError as e:
            names = dict(sigma_iou2="--track_iou2", sigma_iou="--track_iou", sigma_l="--track_low", sigma_h="--track_high",
                         t_min="--track_min_len", max_age="--track_max_age", sigma_d="--track_det", sigma_new="--track_new")
            msg = str(e)
            for k, flag in names.items():
                msg = msg.replace("--track: " + k, flag)
            raise NotImplementedError(msg)
    elif getattr(FLAGS, "track_online", False):
        raise NotImplementedError("--track_online needs --track: it chooses how a live session carries the tracker")
    if getattr(FLAGS, "track_app", False):
        # appearance association is detect_video's, on SORT's cost: refused elsewhere, never ignored
        if not getattr(FLAGS, "track", False) or getattr(FLAGS, "track_method", "iou") != "sort":
            raise NotImplementedError("--track_app needs --track --track_method sort: the fused cost of geometry and appearance is "
                                      "defined for SORT's association alone")
        if not getattr(FLAGS, "stream", False):
            raise NotImplementedError("--track_app needs --stream: the descriptors are pooled from the feature maps net.detect_video "
                                      "holds on the device; the windowed path keeps none")
        if getattr(FLAGS, "live", False):
            raise NotImplementedError("--track_app does not combine with --live: a live session does not carry the descriptors of "
                                      "its frames from push to push")
        if getattr(FLAGS, "seq_nms", False):
            raise NotImplementedError("--track_app does not combine with --seq_nms: Seq-NMS permutes the rows ahead of the tracker, "
                                      "the descriptors belong to the rows as detected")
        if int(FLAGS.window[0]) > 1 and FLAGS.k_join_pos == "late":
            raise NotImplementedError("--track_app does not combine with --k_join_pos %s: the ring of a late join holds the neck's "
                                      "tips, not the backbone's route tensors the descriptor is pooled from" % FLAGS.k_join_pos)
        from viddet_amd.appearance import LEVELS, check_app_params
        a = app_args(FLAGS)
        if isinstance(a["level"], bool) or a["level"] not in LEVELS:
            raise NotImplementedError("--track_app_level must be 8, 16 or 32, got %r" % (a["level"],))
        try:
            check_app_params(a["sigma_app"], a["sigma_prox"], who="--track_app")
        except ValueError as e:
            raise NotImplementedError(str(e).replace("--track_app: sigma_app", "--track_app_cos")
                                      .replace("--track_app: sigma_prox", "--track_app_prox"))
    else:
        for flag, _ in _APP_FLAGS:
            if getattr(FLAGS, flag, None) is not None:
                raise NotImplementedError("--%s needs --track_app: it is a parameter of appearance association" % flag)
    if getattr(FLAGS, "track_gmc", False):
        # camera-motion compensation is detect_video's, on a finished clip: refused elsewhere, never ignored
        if not getattr(FLAGS, "track", False):
            raise NotImplementedError("--track_gmc needs --track: it stabilises the boxes the tracker links")
        if not getattr(FLAGS, "stream", False):
            raise NotImplementedError("--track_gmc needs --stream: the motion is estimated between the consecutive frames of a clip "
                                      "net.detect_video holds; the windowed path sees windows")
        if getattr(FLAGS, "live", False):
            raise NotImplementedError("--track_gmc does not combine with --live: a live session does not carry the signature of "
                                      "its last frame from push to push")
        if getattr(FLAGS, "track_smooth", False):
            raise NotImplementedError("--track_gmc does not combine with --track_smooth: the pass emits boxes, and their way through "
                                      "the stabilised frame has no definition yet")
        if getattr(FLAGS, "tubelet", False):
            raise NotImplementedError("--track_gmc does not combine with --tubelet: the pass emits boxes, and their way through the "
                                      "stabilised frame has no definition yet")
        if getattr(FLAGS, "seq_nms", False):
            raise NotImplementedError("--track_gmc does not combine with --seq_nms: net.detect_video composes the two, the script "
                                      "links the plain rows by a call of its own that knows no camera motion")
        from viddet_amd.motion import check_params as check_gmc
        try:
            check_gmc(who="--track_gmc", **gmc_args(FLAGS))
        except ValueError as e:
            msg = str(e)
            for flag, key in _GMC_FLAGS:
                msg = msg.replace("--track_gmc: " + key, "--" + flag)
            raise NotImplementedError(msg)
    else:
        for flag, _ in _GMC_FLAGS:
            if getattr(FLAGS, flag, None) is not None:
                raise NotImplementedError("--%s needs --track_gmc: it is a parameter of camera-motion compensation" % flag)
    if getattr(FLAGS, "synthetic_pan", 0):
        if FLAGS.synthetic_pan < 0 or len(FLAGS.dataset) > 1:
            raise NotImplementedError("--synthetic_pan takes a step of at least 0 pixels and one dataset, got %d and %d"
                                      % (FLAGS.synthetic_pan, len(FLAGS.dataset)))
    if getattr(FLAGS, "tubelet", False):
        # the tubelet pass runs over the tracks of a finished clip
        if not getattr(FLAGS, "track", False):
            raise NotImplementedError("--tubelet needs --track: the pass runs over the tracks of a clip")
        if getattr(FLAGS, "live", False):
            raise NotImplementedError("--tubelet does not combine with --live: a hole is known only once its track resumes, after "
                                      "the frame has been given out - the pass has no online form")
        if getattr(FLAGS, "seq_nms", False):
            raise NotImplementedError("--tubelet does not combine with --seq_nms: net.detect_video composes the two, the script "
                                      "would need a fourth family of prediction sets")
        if getattr(FLAGS, "tubelet_rescore", "avg") not in ("avg", "max", "none"):
            raise NotImplementedError("--tubelet_rescore must be avg, max or none, got %r" % (FLAGS.tubelet_rescore,))
        from viddet_amd.tubelet import check_params as check_tubelet
        try:
            check_tubelet(who="--tubelet", **tubelet_args(FLAGS))
        except ValueError as e:
            msg = str(e)
            for k, flag in (("max_gap", "--tubelet_max_gap"), ("drop_untracked", "--tubelet_drop_untracked"), ("rescore", "--tubelet_rescore")):
                msg = msg.replace("--tubelet: " + k, flag)
            raise NotImplementedError(msg)
    if getattr(FLAGS, "track_smooth_lag", None) is not None:
        # the fixed-lag form of the smoother is a live session's: refused elsewhere, never ignored
        if not getattr(FLAGS, "live", False):
            raise NotImplementedError("--track_smooth_lag needs --live: it makes the live session (net.open_video) smooth the "
                                      "boxes itself, every frame that many frames late; without --live --track_smooth smooths "
                                      "every clip at its end")
        if not getattr(FLAGS, "track_smooth", False):
            raise NotImplementedError("--track_smooth_lag needs --track_smooth: it chooses how late a live session gives out "
                                      "the smoothed boxes")
        from viddet_amd.smooth_lag import MAX_LAG
        if not 0 <= FLAGS.track_smooth_lag <= MAX_LAG:
            raise NotImplementedError("--track_smooth_lag must be an integer in [0, %d], got %r" % (MAX_LAG, FLAGS.track_smooth_lag))
    if getattr(FLAGS, "track_smooth", False):
        # the smoother runs over the tracks of a finished clip - or, with --track_smooth_lag, of a live session
        if not getattr(FLAGS, "track", False):
            raise NotImplementedError("--track_smooth needs --track: the pass runs over the tracks of a clip")
        if getattr(FLAGS, "live", False) and getattr(FLAGS, "track_smooth_lag", None) is None:
            raise NotImplementedError("--track_smooth does not combine with --live: a frame's smoothed box needs the frames after "
                                      "it - the pass has no online form")
        if getattr(FLAGS, "seq_nms", False):
            raise NotImplementedError("--track_smooth does not combine with --seq_nms: net.detect_video composes the two, the "
                                      "script would need a further family of prediction sets")
        if getattr(FLAGS, "tubelet", False):
            raise NotImplementedError("--track_smooth does not combine with --tubelet: net.detect_video composes the two, the "
                                      "script keeps one extra family of files at a time")
        from viddet_amd.smooth import check_params as check_smooth
        try:
            check_smooth(who="--track_smooth", **smooth_args(FLAGS))
        except ValueError as e:
            raise NotImplementedError(str(e).replace("--track_smooth: max_gap", "--track_smooth_gap"))
    if getattr(FLAGS, "track_stitch", False):
        # the stitching pass runs over the tracks of a finished clip
        if not getattr(FLAGS, "track", False):
            raise NotImplementedError("--track_stitch needs --track: the pass runs over the tracks of a clip")
        if getattr(FLAGS, "live", False):
            raise NotImplementedError("--track_stitch does not combine with --live: a fragment's successor is known only later - "
                                      "the pass has no online form")
        if getattr(FLAGS, "seq_nms", False):
            raise NotImplementedError("--track_stitch does not combine with --seq_nms: net.detect_video composes the two, the "
                                      "script would need a further family of tracked twins")
        if getattr(FLAGS, "tubelet", False):
            raise NotImplementedError("--track_stitch does not combine with --tubelet: net.detect_video composes the two, the "
                                      "script keeps one extra family of files at a time")
        if getattr(FLAGS, "track_smooth", False):
            raise NotImplementedError("--track_stitch does not combine with --track_smooth: net.detect_video composes the two, "
                                      "the script keeps one extra family of files at a time")
        from viddet_amd.stitch import check_params as check_stitch
        try:
            check_stitch(who="--track_stitch", **stitch_args(FLAGS))
        except ValueError as e:
            raise NotImplementedError(str(e).replace("--track_stitch: max_gap", "--track_stitch_gap")
                                      .replace("--track_stitch: sigma_iou", "--track_stitch_iou"))
    else:
        for flag in ("track_stitch_gap", "track_stitch_iou"):
            if getattr(FLAGS, flag, None) is not None:
                raise NotImplementedError("--%s needs --track_stitch: it is a parameter of that pass" % flag)
    if getattr(FLAGS, "visualise", False):
        # the overlay is drawn by net.detect_video on a clip's own frames
        if not getattr(FLAGS, "stream", False):
            raise NotImplementedError("--visualise needs --stream: the overlay is drawn by net.detect_video on a clip's frames; "
                                      "the windowed path hands out windows, not frames")
        if getattr(FLAGS, "live", False):
            raise NotImplementedError("--visualise does not combine with --live: a live session gives its frames back before "
                                      "their rows are final, it would have to hold them")
        if len(FLAGS.dataset) > 1:
            raise NotImplementedError("--visualise takes one --dataset name: the combined set has no clips")
        for flag, lo, hi in (("vis_thickness", 1, 8), ("vis_scale", 1, 4), ("vis_trail", 0, 16), ("vis_every", 1, 1 << 30)):
            v = getattr(FLAGS, flag, None)
            if v is not None and not lo <= int(v) <= hi:
                raise NotImplementedError("--%s must lie in [%d, %d], got %r" % (flag, lo, hi, v))
    else:
        for flag in ("vis_thickness", "vis_scale", "vis_trail", "vis_every"):
            if getattr(FLAGS, flag, None) is not None:
                raise NotImplementedError("--%s needs --visualise: it is a parameter of the overlay" % flag)
    # accepted for command-line compatibility, refused when they would change the result (never silently ignored):
    # research variants, the VID metric's options, evaluation on another dataset's class list
    for flag in ("temp", "mult_out", "new_model", "motion_stream", "offset", "per_frame_metric",
                 "worst_video_path", "trained_on"):
        v = getattr(FLAGS, flag)
        if v and not (isinstance(v, str) and not v.strip()):
            raise NotImplementedError("--%s is outside the yolo3_darknet53 hot path" % flag)
    vid = "vid" in [m.lower() for m in (getattr(FLAGS, "metrics", None) or [])]
    coco = "coco" in [m.lower() for m in (getattr(FLAGS, "metrics", None) or [])]
    if FLAGS.model_agnostic:
        FLAGS.metric_agnostic = True                      # detect_yolo3.py:797-798
    elif FLAGS.metric_agnostic and not (vid or mot or hota):
        raise NotImplementedError("--metric_agnostic without --model_agnostic only acts inside VIDDetectionMetric and MOTMetric "
                                  "(detect_yolo3.py:189-190): it needs --metrics vid or --metrics mot (or --metrics hota: "
                                  "HOTAMetric), the voc metric takes no agnostic argument")
    if vid and len(FLAGS.dataset) > 1:
        raise NotImplementedError("--metrics vid does not combine with several --dataset names: the combined set has no "
                                  "tracks, so no motion IoUs")
    if getattr(FLAGS, "device_metric", False) and not (vid or coco or mot or hota):
        raise NotImplementedError("--device_metric acts on --metrics vid, --metrics coco, --metrics mot and --metrics hota only "
                                  "(train_yolov3.py has the voc metric's)")
    # detect_yolo3.py:795,872-882: conv_types[0] != 2 selects yolo3_3ddarknet(classes, conv_types=...) and nothing else
    ct = check_conv_types(FLAGS.conv_types, FLAGS.window[0])
    if ct is not None:
        for flag, on in (("k_join_type", FLAGS.k_join_type), ("k_join_pos", FLAGS.k_join_pos), ("rnn_pos", FLAGS.rnn_pos),
                         ("corr_pos", FLAGS.corr_pos), ("precision", FLAGS.precision == "bf16"),
                         ("block_conv_type", FLAGS.block_conv_type != "2")):
            if on:
                raise NotImplementedError("--%s does not combine with --conv_types %s: yolo3_3ddarknet is not passed it (its "
                                          "neck is the single-frame one; the temporal-conv kernels are fp32)"
                                          % (flag, ",".join(str(c) for c in ct)))
        if FLAGS.model_agnostic:
            raise NotImplementedError("--model_agnostic does not combine with --conv_types %s: yolo3_3ddarknet is built "
                                      "without the flag (detect_yolo3.py:872-882)" % ",".join(str(c) for c in ct))
    if FLAGS.model_agnostic and FLAGS.rnn_pos == "out":
        raise NotImplementedError("--model_agnostic with --rnn_pos out: the RNN output block is a tail of its own that is not "
                                  "built agnostic")
    if getattr(FLAGS, "frame_format", "rgb") == "nv12":
        if not getattr(FLAGS, "device_resize", False):
            raise NotImplementedError("--frame_format nv12 needs --device_resize: NV12 frames are converted inside the kernel "
                                      "that resizes them, the host resize has no NV12 path")
        if len(FLAGS.dataset) > 1:
            raise NotImplementedError("--frame_format nv12 does not combine with several --dataset names: the combined set's "
                                      "path is left on the host resize")
    if getattr(FLAGS, "device_resize", False) and len(FLAGS.dataset) > 1:
        raise NotImplementedError("--device_resize does not combine with several --dataset names: the combined set's path is "
                                  "left on the host resize")
    if getattr(FLAGS, "stream", False):
        # net.detect_video runs the per-frame part of the network once per frame: what mixes the frames of a window ahead
        # of the join has no such part (YOLOV3._stream_refusal names the same reasons)
        for flag, on, why in (
                ("conv_types", ct is not None, "the (2+1)-D backbone mixes the frames of a window inside the backbone"),
                ("corr_pos", FLAGS.corr_pos, "the correlation join compares every frame with its window's centre frame and has "
                                             "no form that reads the feature ring"),
                ("rnn_pos", FLAGS.rnn_pos, "the ConvGRU carries a state across the frames of a window ahead of the join"),
                ("block_conv_type", FLAGS.block_conv_type != "2", "the neck's 3-D / 2+1-D convs mix the frames of a window ahead "
                                                                  "of the late join"),
                ("dataset", len(FLAGS.dataset) > 1, "the combined set has no clips")):
            if on:
                raise NotImplementedError("--stream does not combine with --%s: %s" % (flag, why))
        if int(FLAGS.window[0]) > 1 and (FLAGS.k_join_type not in ("max", "mean", "cat") or FLAGS.k_join_pos not in ("early", "late")):
            raise NotImplementedError("--stream with --window %s needs --k_join_type max|mean|cat and --k_join_pos early|late: "
                                      "the graph is split at that join" % FLAGS.window[0])
    return ct


def save_predictions(save_dir, dataset, boxes, overwrite=True, max_do=-1):
    """detect_yolo3.py:275-330: one text file per image, lines `path,id,score,x1,y1,x2,y2`."""
    os.makedirs(save_dir, exist_ok=True)
    n = len(dataset) if max_do < 0 else min(max_do, len(dataset))
    for idx in range(n):
        img_path = dataset.sample_path(idx)
        file_id = os.path.split(img_path)[1].split(".")[0]
        out = os.path.join(save_dir, file_id + ".txt")
        if os.path.exists(out) and not overwrite:
            continue
        with open(out, "w") as f:
            for box in boxes.get(img_path, []):
                f.write("{},{},{},{},{},{},{}\n".format(img_path, box[0], box[1], box[2], box[3], box[4], box[5]))


def load_predictions(save_dir, dataset, max_do=-1):
    """detect_yolo3.py:333-400 (plain, non-agnostic branch)."""
    boxes = dict()
    n = len(dataset) if max_do < 0 else min(max_do, len(dataset))
    for idx in range(n):
        img_path = dataset.sample_path(idx)
        file_id = os.path.split(img_path)[1].split(".")[0]
        p = os.path.join(save_dir, file_id + ".txt")
        if not os.path.exists(p):
            continue
        with open(p) as f:
            for line in f:
                v = line.rstrip().split(",")
                boxes.setdefault(v[0], []).append([int(v[1])] + [float(t) for t in v[2:7]])
    return boxes


def evaluate(metrics, dataset, predictions, data_shape):
    """detect_yolo3.py:659-695: feed saved predictions and (resized, normalised) ground truth to the metrics."""
    tf = YOLO3VideoInferenceTransform(data_shape, data_shape)
    if getattr(dataset, "frame_format", "rgb") == "nv12":      # only the resized boxes are used: the NV12 frames pass through
        tf = YOLO3VideoInferenceTransform(data_shape, data_shape, device_normalize=True, device_resize=True, frame_format="nv12")
    for idx in range(len(dataset)):
        img, label = dataset[idx]
        _, gt, _ = tf(img, label, idx)
        gt_boxes = gt[:, :4] / data_shape
        pred = np.asarray(predictions.get(dataset.sample_path(idx), np.zeros((0, 6))), dtype=np.float64).reshape(-1, 6)
        for m in metrics:
            m.update([pred[:, 2:6]], [pred[:, 0]], [pred[:, 1]], [gt_boxes], [gt[:, 4]], [gt[:, 5]])
    return [m.get() for m in metrics]


def evaluate_by_sample_id(metric, dataset, predictions):
    """detect_yolo3.py:659-695 for the metrics that take their ground truth from the dataset itself (vid, coco): the saved
    predictions, un-normalised to the source frame (:685-688), filed under the image's sample id; an image without a saved
    detection is not visited, as there"""
    for idx, sid in enumerate(dataset.sample_ids):
        img_path = dataset.sample_path(idx)
        if img_path in predictions:
            w, h = dataset.image_size(sid)
            pred = predictions[img_path]
            det_bboxes = [[[[b[2] * w, b[3] * h, b[4] * w, b[5] * h] for b in pred]]]          # [1][image][row][4]
            metric.update(det_bboxes, [[[b[0] for b in pred]]], [[[b[1] for b in pred]]], None, None, None, sid=sid)
    return metric.get()


evaluate_vid = evaluate_by_sample_id          # its name while vid was the only such metric


def write_results(path, names, values, echo=True):
    """detect_yolo3.py:920-931: `name value` per line"""
    with open(path, "w") as f:
        for k, v in zip(names, values):
            if echo:
                print(k, v)
            f.write("{} {}\n".format(k, v))


def main(argv=None):
    FLAGS = parse_flags(argv)
    FLAGS.window = [int(s) for s in FLAGS.window]
    if FLAGS.window[0] == 1:
        FLAGS.k_join_type = FLAGS.k_join_pos = None
    ct = check_flags(FLAGS)
    rank, world = vdist.init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("detect_yolo3.py needs an MI355X: the HIP path has no CPU fallback")
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    name = FLAGS.dataset[0]
    # --frame_format nv12: the synthetic sets hand out their frames as a decoder would (video.rgb_to_nv12)
    fmt = dict(frame_format="nv12", yuv_matrix=FLAGS.yuv_matrix, yuv_range=FLAGS.yuv_range) if FLAGS.frame_format == "nv12" else {}
    if len(FLAGS.dataset) > 1:          # detect_yolo3.py:166-167: several datasets = the combined set with its class tree
        dataset = SyntheticCombined(FLAGS.dataset, num_samples=FLAGS.synthetic_samples, classes_per_set=FLAGS.synthetic_classes)
    elif FLAGS.synthetic_pan > 0:
        # SyntheticTracks under a moving camera: steps of up to --synthetic_pan pixels, multiples of --track_gmc_cell
        cell = 4 if FLAGS.track_gmc_cell is None else FLAGS.track_gmc_cell
        dataset = SyntheticPan(name, num_videos=2 if FLAGS.synthetic_videos is None else FLAGS.synthetic_videos,
                               frames_per_video=FLAGS.synthetic_samples, window=FLAGS.window[0],
                               step=FLAGS.window[1] if len(FLAGS.window) > 1 else 1, pan=max(FLAGS.synthetic_pan, cell), cell=cell, **fmt)
    elif {"vid", "mot", "hota"} & {m.lower() for m in FLAGS.metrics}:
        # the vid, mot and hota metrics need tracks: clips as below, whose labels are moving objects with track ids and motion IoUs
        dataset = SyntheticTracks(name, num_videos=2 if FLAGS.synthetic_videos is None else FLAGS.synthetic_videos,
                                  frames_per_video=FLAGS.synthetic_samples, window=FLAGS.window[0],
                                  step=FLAGS.window[1] if len(FLAGS.window) > 1 else 1, **fmt)
    elif FLAGS.stream or FLAGS.synthetic_videos is not None:
        # clips: --synthetic_videos of them (given, or 2 with --stream), --synthetic_samples frames each, windows by --window K,step
        dataset = SyntheticVideo(name, num_videos=2 if FLAGS.synthetic_videos is None else FLAGS.synthetic_videos,
                                 frames_per_video=FLAGS.synthetic_samples, window=FLAGS.window[0],
                                 step=FLAGS.window[1] if len(FLAGS.window) > 1 else 1, **fmt)
    else:
        # --window k: a sample is the k-frame window around the frame the rows belong to (as train_yolov3.py's sets)
        dataset = SyntheticDetection(name, num_samples=FLAGS.synthetic_samples, window=FLAGS.window[0], **fmt)
    # frames travel as uint8 and are normalised on the device (vd_preprocess_u8_nchw: the transform's own arithmetic)
    # (--device_resize: at their source size, resized there too - vd_resize_u8_nchw, NV12 frames vd_resize_nv12_nchw)
    loader = Loader(dataset, YOLO3VideoInferenceTransform(FLAGS.data_shape, FLAGS.data_shape, device_normalize=True,
                                                          device_resize=FLAGS.device_resize, frame_format=FLAGS.frame_format),
                    FLAGS.batch_size, train=False, last_batch="keep", rank=rank, world=world)
    # detect_yolo3.py:871-892
    if ct is not None:
        net = yolo3_3ddarknet(dataset.classes, pretrained_base=False, conv_types=ct, k=FLAGS.window[0])
    else:
        net = yolo3_darknet53(dataset.classes, pretrained_base=False, k=FLAGS.window[0], k_join_type=FLAGS.k_join_type,
                              k_join_pos=FLAGS.k_join_pos, block_conv_type=FLAGS.block_conv_type,
                              corr_pos=FLAGS.corr_pos or None, corr_d=FLAGS.corr_d, rnn_pos=FLAGS.rnn_pos or None,
                              agnostic=FLAGS.model_agnostic)
    if FLAGS.random_init:
        net.initialize(init="he", obj_bias=-2.0)
    else:
        net.load_parameters(FLAGS.model_path)
    net.set_precision(FLAGS.precision)
    if FLAGS.device_resize and FLAGS.frame_format == "nv12":
        net.set_device_resize(FLAGS.data_shape, FLAGS.data_shape, source="nv12", matrix=FLAGS.yuv_matrix, range=FLAGS.yuv_range)
    elif FLAGS.device_resize:
        net.set_device_resize(FLAGS.data_shape, FLAGS.data_shape)
    save_dir = pred_dir(FLAGS.save_dir, FLAGS.save_prefix, FLAGS.model_agnostic)
    seq = seq_nms_args(FLAGS)
    seq_kw = {} if seq is None else dict(seq_nms=seq, input_nms=FLAGS.seq_nms_input_nms)
    if seq is not None and not FLAGS.stream and world > 1:
        raise NotImplementedError("--seq_nms without --stream runs on one GPU: the windowed path shards the frames of a clip "
                                  "over the ranks")
    trk = track_args(FLAGS)
    if trk is not None:
        seq_kw = dict(seq_kw, track=trk)
        if not FLAGS.stream and world > 1:
            raise NotImplementedError("--track without --stream runs on one GPU: the windowed path shards the frames of a clip "
                                      "over the ranks")
    tub = tubelet_args(FLAGS)
    if tub is not None:
        seq_kw = dict(seq_kw, tubelet=tub)
    smo = smooth_args(FLAGS)
    if smo is not None:
        seq_kw = dict(seq_kw, smooth=smo)
    sti = stitch_args(FLAGS)
    if sti is not None:
        seq_kw = dict(seq_kw, stitch=sti)
    motion_log = [] if trk is not None and "gmc" in trk else None
    if FLAGS.stream:
        boxes = detect_stream(net, dataset, FLAGS.data_shape, FLAGS.window[1] if len(FLAGS.window) > 1 else 1, FLAGS.batch_size,
                              FLAGS.max_do, rank, world, device_resize=FLAGS.device_resize, frame_format=FLAGS.frame_format,
                              live=FLAGS.live_push if FLAGS.live else None, track_online=FLAGS.track_online,
                              smooth_lag=FLAGS.track_smooth_lag, visualise=visualise_args(FLAGS, dataset), motion_log=motion_log, **seq_kw)
    else:
        boxes = detect(net, dataset, loader, FLAGS.max_do, FLAGS.data_shape if FLAGS.device_resize else None, **seq_kw)
    boxes_seq = tracks = tracks_seq = boxes_tub = tracks_tub = None
    if tub is not None or smo is not None or sti is not None:              # check_flags: one of the three at most
        boxes, boxes_seq, tracks, tracks_seq, boxes_tub, tracks_tub = boxes
    elif trk is not None:
        boxes, boxes_seq, tracks, tracks_seq = boxes
    elif seq is not None:
        boxes, boxes_seq = boxes
    if world > 1:
        # frames are sharded over the ranks (replicas, no collective on the data path); the per-image box lists (host
        # objects) are merged so that ONE rank writes every file - a rank must never write an (empty) file for an image
        # another rank detected on - and evaluates the whole set as the reference's single process does
        merged = dict()
        for part in vdist.all_gather_objects(boxes):
            merged.update(part)
        boxes = merged
        if boxes_seq is not None:
            merged = dict()
            for part in vdist.all_gather_objects(boxes_seq):
                merged.update(part)
            boxes_seq = merged
        if trk is not None:
            gathered = []
            for part_of in (tracks, tracks_seq, boxes_tub, tracks_tub):
                merged = None
                if part_of is not None:
                    merged = dict()
                    for part in vdist.all_gather_objects(part_of):
                        merged.update(part)
                gathered.append(merged)
            tracks, tracks_seq, boxes_tub, tracks_tub = gathered
        if motion_log is not None:
            motion_log = sorted(row for part in vdist.all_gather_objects(motion_log) for row in part)
        if rank != 0:
            return None
    result = save_and_evaluate(FLAGS, dataset, boxes, save_dir)
    if motion_log is not None:
        # --track_gmc: the camera's motion beside everything the run without it writes
        with open(os.path.join(FLAGS.save_dir, FLAGS.save_prefix, "motion.txt"), "w") as f:
            for row in motion_log:
                f.write("%d %d %d %d %d %d\n" % row)
    if boxes_seq is not None:
        # the rescored predictions and their results beside the plain ones: pred_seq, vid_seq.txt, coco_seq.txt, ...
        save_and_evaluate(FLAGS, dataset, boxes_seq, pred_dir(FLAGS.save_dir, FLAGS.save_prefix, FLAGS.model_agnostic, seq=True),
                          seq=True)
    if trk is not None:
        # the tracked twins, after everything a run without --track writes: pred_trk / tracks.txt, pred_seq_trk / tracks_seq.txt
        # (and with --metrics mot / hota their mot.txt / mot_seq.txt, hota.txt / hota_seq.txt; the plain twin's - mot's where
        # both ran - is what main() returns where no other metric ran)
        for bx, tr, is_seq in ((boxes, tracks, False), (boxes_seq, tracks_seq, True)):
            if bx is not None:
                mot_result = save_tracks(FLAGS, dataset, bx, tr, is_seq)
                if result is None and not is_seq:
                    result = mot_result
    if boxes_tub is not None:
        # the rows after the tubelet pass, last: pred_tub, vid_tub.txt, coco_tub.txt, ..., pred_tub_trk, tracks_tub.txt
        # (--track_smooth: the rows with their smoothed boxes, pred_smo, vid_smo.txt, ..., pred_smo_trk, tracks_smo.txt)
        tail = True if tub is not None else "smo"
        save_and_evaluate(FLAGS, dataset, boxes_tub, pred_dir(FLAGS.save_dir, FLAGS.save_prefix, FLAGS.model_agnostic, tub=tail),
                          tub=tail)
        save_tracks(FLAGS, dataset, boxes_tub, tracks_tub, tub=tail)
    if sti is not None:
        # the plain rows under their stitched ids, last: pred_sti_trk, tracks_sti.txt, mot_sti.txt, hota_sti.txt
        save_tracks(FLAGS, dataset, boxes, tracks_tub, tub="sti")
    return result


def save_tracks(FLAGS, dataset, boxes, tracks, seq=False, tub=False):
    """--track: the twin of a prediction set - its files' lines with `,track` appended (every row, -1 too) - and one line
    `clip tracks rows mean_len` per clip in tracks.txt / tracks_seq.txt (tub: pred_tub_trk, tracks_tub.txt; 'smo':
    pred_smo_trk, tracks_smo.txt; 'sti': the plain rows under the ids of --track_stitch, pred_sti_trk, tracks_sti.txt)"""
    save_dir = pred_dir(FLAGS.save_dir, FLAGS.save_prefix, FLAGS.model_agnostic, seq=seq, trk=True, tub=tub)
    os.makedirs(save_dir, exist_ok=True)
    n = len(dataset) if FLAGS.max_do < 0 else min(FLAGS.max_do, len(dataset))
    per_clip = [[set(), 0] for _ in range(dataset.num_videos)]
    for idx in range(n):
        img_path = dataset.sample_path(idx)
        file_id = os.path.split(img_path)[1].split(".")[0]
        rows, ids = boxes.get(img_path, []), tracks.get(img_path, [])
        assert len(rows) == len(ids), "a track id per saved row"
        with open(os.path.join(save_dir, file_id + ".txt"), "w") as f:
            for box, tid in zip(rows, ids):
                f.write("{},{},{},{},{},{},{},{}\n".format(img_path, box[0], box[1], box[2], box[3], box[4], box[5], tid))
                if tid >= 0:
                    per_clip[idx // dataset.frames_per_video][0].add(tid)
                    per_clip[idx // dataset.frames_per_video][1] += 1
    out = os.path.join(FLAGS.save_dir, FLAGS.save_prefix, result_name("tracks", FLAGS.model_agnostic, seq=seq, tub=tub) + ".txt")
    with open(out, "w") as f:
        for v, (ids, rows) in enumerate(per_clip):
            f.write("{} {} {} {:.4f}\n".format(v, len(ids), rows, rows / len(ids) if ids else 0.0))
    metrics = [m.lower() for m in FLAGS.metrics]
    if "mot" not in metrics and "hota" not in metrics:
        return None
    # --metrics mot / hota: what is scored is what is on disk - the rows read back from the twin's files
    preds = load_tracked_predictions(save_dir, dataset, FLAGS.max_do)
    result = None
    if "mot" in metrics:
        if FLAGS.device_metric:
            from viddet_amd.device_mot_metric import DeviceMOTMetric as mot_class
        else:
            mot_class = MOTMetric
        result = evaluate_tracks(mot_class(dataset, iou_thresh=0.5, agnostic=FLAGS.metric_agnostic), dataset, preds)
        # mot.txt / mot_seq.txt / mot_tub.txt, mot_ag*.txt under --model_agnostic, mot_ag_met*.txt under --metric_agnostic alone
        write_results(os.path.join(FLAGS.save_dir, FLAGS.save_prefix,
                                   result_name("mot", FLAGS.model_agnostic, FLAGS.metric_agnostic, seq, tub) + ".txt"), *result)
    if "hota" in metrics:
        if FLAGS.device_metric:
            from viddet_amd.device_hota_metric import DeviceHOTAMetric as hota_class
        else:
            hota_class = HOTAMetric
        hota_result = evaluate_tracks(hota_class(dataset, agnostic=FLAGS.metric_agnostic), dataset, preds)
        # hota.txt / hota_seq.txt / hota_tub.txt, hota_ag*.txt, hota_ag_met*.txt: named as mot's
        write_results(os.path.join(FLAGS.save_dir, FLAGS.save_prefix,
                                   result_name("hota", FLAGS.model_agnostic, FLAGS.metric_agnostic, seq, tub) + ".txt"), *hota_result)
        result = hota_result if result is None else result
    return result


def load_tracked_predictions(save_dir, dataset, max_do=-1):
    """load_predictions for a tracked twin: {image path: [[id, score, x1, y1, x2, y2, track]]}"""
    boxes = dict()
    n = len(dataset) if max_do < 0 else min(max_do, len(dataset))
    for idx in range(n):
        img_path = dataset.sample_path(idx)
        p = os.path.join(save_dir, os.path.split(img_path)[1].split(".")[0] + ".txt")
        if not os.path.exists(p):
            continue
        with open(p) as f:
            for line in f:
                v = line.rstrip().split(",")
                boxes.setdefault(v[0], []).append([int(v[1])] + [float(t) for t in v[2:7]] + [int(v[7])])
    return boxes


def evaluate_tracks(metric, dataset, predictions):
    """evaluate_by_sample_id for the MOT metric: the saved rows of a tracked twin, un-normalised to the source frame in the same
    way, with their track ids; an image without a saved row is not fed - the metric takes it as a frame without predictions"""
    for idx, sid in enumerate(dataset.sample_ids):
        img_path = dataset.sample_path(idx)
        if img_path in predictions:
            w, h = dataset.image_size(sid)
            pred = predictions[img_path]
            det_bboxes = [[[[b[2] * w, b[3] * h, b[4] * w, b[5] * h] for b in pred]]]          # [1][image][row][4]
            metric.update(det_bboxes, [[[b[0] for b in pred]]], [[[b[1] for b in pred]]], None, None, None, sid=sid,
                          tracks=[[[b[6] for b in pred]]])
    return metric.get()


def save_and_evaluate(FLAGS, dataset, boxes, save_dir, seq=False, tub=False):
    """The tail of main(): the prediction files under save_dir, then --metrics on what was saved; seq names the result files
    of the predictions rescored by --seq_nms, tub those of the rows after the pass of --tubelet ('smo': of --track_smooth)."""
    save_predictions(save_dir, dataset, boxes, max_do=FLAGS.max_do)
    metrics = [m.lower() for m in FLAGS.metrics]
    out_dir = os.path.join(FLAGS.save_dir, FLAGS.save_prefix)
    preds = load_predictions(save_dir, dataset, FLAGS.max_do) if {"vid", "voc", "coco"} & set(metrics) else None
    vid_result = voc_result = coco_result = None
    if "vid" in metrics:
        if FLAGS.device_metric:
            from viddet_amd.device_vid_metric import DeviceVIDDetectionMetric as vid_class
        else:
            vid_class = VIDDetectionMetric
        vid_result = evaluate_by_sample_id(vid_class(dataset, iou_thresh=0.5, agnostic=FLAGS.metric_agnostic), dataset, preds)
        # vid.txt / vid_ag.txt / vid_ag_met.txt
        write_results(os.path.join(out_dir, result_name("vid", FLAGS.model_agnostic, FLAGS.metric_agnostic, seq, tub) + ".txt"),
                      *vid_result)
    if len(FLAGS.dataset) > 1 and {"voc", "coco"} & set(metrics):              # detect_yolo3.py:898-899 (class-tree sets), ahead of
        preds = hierarchical_nms(preds, dataset, level_thresh=FLAGS.hier_level)  # the metrics (vid is refused on such a set)
    if "voc" in metrics:
        (names, values), = evaluate([VOCMApMetric(iou_thresh=0.5, class_names=dataset.classes)], dataset, preds,
                                    FLAGS.data_shape)
        print("{}={:.4f}".format(names[-1], values[-1]))
        if FLAGS.model_agnostic:
            # the per-class and the mean AP in <metric>_ag.txt beside pred_ag.  The metric is handed the rows as they are (ids
            # all 0): the reference's voc / coco metrics take no agnostic argument
            write_results(os.path.join(out_dir, result_name("voc", True, seq=seq, tub=tub) + ".txt"), names, values, echo=False)
        voc_result = names, values
    if "coco" in metrics:
        if FLAGS.device_metric:
            from viddet_amd.device_coco_metric import DeviceCOCODetectionMetric as coco_class
        else:
            coco_class = COCODetectionMetric
        # get_metric :186: the detections' JSON beside pred/, removed again (cleanup); no time stamp in its name
        metric = coco_class(dataset, os.path.join(out_dir, "coco_results" + ("_seq" if seq else "") + _pass_tail(tub)), use_time=False, cleanup=True, data_shape=None)
        coco_result = evaluate_by_sample_id(metric, dataset, preds)
        write_results(os.path.join(out_dir, result_name("coco", FLAGS.model_agnostic, FLAGS.metric_agnostic, seq, tub) + ".txt"),
                      *coco_result)
    # what main() hands back is what it handed back before coco was built: voc's where asked for, else vid's; coco's alone
    if voc_result is not None:
        return voc_result
    return vid_result if vid_result is not None else coco_result


if __name__ == "__main__":
    main()
