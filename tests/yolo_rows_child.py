"""Child process of tests/test_yolo_edges_gpu.py::test_decode_rows_form: the row-streaming decode (VD_DECODE_ROWS=1, read once
per process by the library) over every fixture of tests/yolo_edge_fixtures.DECODE_CASES, candidates written to an .npz.

    python -m tests.yolo_rows_child OUT.npz"""
import os
import sys

import numpy as np
import torch

from oracle import yolo as Y
from tests import yolo_edge_fixtures as F
from tests.util import nchw_to_dev_nhwc


def decode_candidates(ops, fx):
    """one vd_yolo_decode_filter launch with room for every row; per image (rows ascending, their scores)"""
    hd = [nchw_to_dev_nhwc(h, fx.ldh) for h in fx.heads]
    h = ops.make_head_desc(hd, fx.grids, fx.ldh, Y.OUT_STRIDES, Y.OUT_ANCHORS, fx.b, fx.c)
    cap = fx.c * 3 * sum(g * g for g in fx.grids)
    cs = torch.full((fx.b, cap), -7.0, device="cuda")
    cr = torch.full((fx.b, cap), -7, dtype=torch.int32, device="cuda")
    cnt = torch.empty(fx.b, dtype=torch.int32, device="cuda")
    ops.yolo_decode_filter(h, F.VALID_T, cs, cr, cap, cnt)
    torch.cuda.synchronize()
    out = []
    for bi in range(fx.b):
        n = int(cnt[bi])
        assert 0 <= n <= cap
        rows, sc = cr[bi, :n].cpu().numpy(), cs[bi, :n].cpu().numpy()
        assert n == cap or (int(cr[bi, n:].max()) == -7 and float(cs[bi, n:].max()) == -7.0), "slots beyond the count were written"
        o = np.argsort(rows, kind="stable")
        out.append((rows[o], sc[o]))
    return out


def main(path):
    assert os.environ.get("VD_DECODE_ROWS") == "1"
    from viddet_amd import ops
    res = {}
    for name in sorted(F.DECODE_CASES):
        for bi, (rows, sc) in enumerate(decode_candidates(ops, F.decode_fixture(name))):
            res["%s_rows%d" % (name, bi)] = rows
            res["%s_score%d" % (name, bi)] = sc
    np.savez(path, **res)


if __name__ == "__main__":
    main(sys.argv[1])
