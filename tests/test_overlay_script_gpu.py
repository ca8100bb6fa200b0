"""detect_yolo3.py --stream --visualise on the GPU: the PPM files it writes are overlay_host of the rows it saves,
byte for byte, and every other file is the one the run without the flag writes."""
import os

import numpy as np
import pytest

from viddet_amd import overlay as O

pytestmark = pytest.mark.gpu


def test_detect_script_visualise(tmp_path):
    import detect_yolo3 as D
    from viddet_amd.data import SyntheticTracks
    T, W, every = 5, 64, 2
    common = ["--random_init", "--dataset", "vid", "--synthetic_samples", str(T), "--synthetic_videos", "1", "--data_shape", str(W),
              "--batch_size", "2", "--metrics", "vid", "--save_dir", str(tmp_path), "--stream", "--device_resize", "--track",
              "--track_high", "0", "--track_max_age", "2", "--detection_threshold", "0.02"]     # (a random model's scores are low)
    D.main(common + ["--save_prefix", "p"])
    D.main(common + ["--save_prefix", "q", "--visualise", "--display_gt", "--vis_every", str(every), "--vis_trail", "3"])
    p, q = tmp_path / "p", tmp_path / "q"
    made = sorted(os.listdir(p))
    assert sorted(os.listdir(q)) == sorted(made + ["vis"])
    for name in made:                                                      # everything a run without --visualise writes, byte for byte
        if os.path.isdir(p / name):
            assert sorted(os.listdir(p / name)) == sorted(os.listdir(q / name))
            for f in os.listdir(p / name):
                assert open(p / name / f, "rb").read() == open(q / name / f, "rb").read(), (name, f)
        else:
            assert open(p / name, "rb").read() == open(q / name, "rb").read(), name
    assert os.listdir(q / "vis") == ["0000"]
    assert sorted(os.listdir(q / "vis" / "0000")) == ["%06d.ppm" % t for t in range(0, T, every)]
    # the picture: overlay_host on the rows `pred_trk` holds (--data_shape 64: the saved box * 64 is the box, exactly; the saved
    # rows are clipped to the image, which moves no pixel box, and rows without a class are left out, which keeps the order)
    ds = SyntheticTracks("vid", num_videos=1, frames_per_video=T, window=1, step=1)
    order = [os.path.split(ds.sample_path(i))[1].split(".")[0] + ".txt" for i in range(T)]
    lines = [open(q / "pred_trk" / f).read().splitlines() for f in order]
    N = max(1, max(len(l) for l in lines))
    ids, scores, bboxes = -np.ones((T, N), np.float32), -np.ones((T, N), np.float32), -np.ones((T, N, 4), np.float32)
    track = -np.ones((T, N), np.int32)
    for t, l in enumerate(lines):
        for i, line in enumerate(l):
            v = line.split(",")
            ids[t, i], scores[t, i], track[t, i] = int(v[1]), np.float32(v[2]), int(v[7])
            bboxes[t, i] = np.asarray([np.float32(c) for c in v[3:7]], np.float32) * np.float32(W)
    w0, h0 = ds.frame_size
    labels = [ds[i][1] for i in range(T)]
    gt = np.full((T, max(len(r) for r in labels), 5), -1.0, np.float32)
    for t, r in enumerate(labels):
        gt[t, :len(r), :4] = r[:, :4] * (W / w0, W / h0, W / w0, W / h0)   # the labels scaled as the predictions are
        gt[t, :len(r), 4] = r[:, 4]
    frames = ds.video_frames(0)
    assert frames.shape == (T, h0, w0, 3)
    want, painted = O.overlay_host(frames, ids, scores, bboxes, track, gt, net_size=(W, W), thresh=0.02, trail=3, class_names=tuple(ds.classes))
    assert painted.min() > 0 and (scores >= 0.02).sum() > 10, "fixture produced (almost) no rows to draw"
    for t in range(0, T, every):
        got = open(q / "vis" / "0000" / ("%06d.ppm" % t), "rb").read()
        assert got == b"P6\n%d %d\n255\n" % (w0, h0) + want[t].tobytes(), t
    print("painted", painted.tolist(), "rows drawn:", int((scores >= 0.02).sum()))
