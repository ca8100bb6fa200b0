"""CPU: the host side of bf16-storage training for temporal windows - the three entry points the library gained, the ABI
revision, and which networks set_storage('bf16') accepts."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vd_temporal_pool_train_bf16", "vd_temporal_pool_bwd_bf16", "vd_corr_bwd_bf16")


def test_library_exports_the_join_training_kernels_at_abi_8():
    from viddet_amd import lib as L
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "viddet_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
    assert lib.vd_abi_version() == L.ABI_VERSION == 8
    # argument checks run before any launch: no GPU is touched
    assert lib.vd_temporal_pool_train_bf16(None, None, None, 1, 3, 8, 0, None) == -1
    assert b"vd_temporal_pool_train_bf16" in lib.vd_last_error()
    assert lib.vd_temporal_pool_bwd_bf16(16, None, 16, 1, 3, 8, 0, None) == -1        # the max needs its winners
    assert lib.vd_temporal_pool_bwd_bf16(16, 16, 16, 1, 3, 12, 0, None) == -1          # inner % 8
    assert lib.vd_corr_bwd_bf16(16, 16, 16, 1, 3, 4, 4, 48, 1, 192, None) == -1
    assert b"multiple of 32" in lib.vd_last_error()
    assert lib.vd_corr_bwd_bf16(16, 16, 16, 1, 3, 4, 4, 32, 2, 128, None) == -1        # ldy < Cc = 96 + 50
    assert b"ldy" in lib.vd_last_error()


def _net(**kw):
    from viddet_amd.model import yolo3_darknet53
    return yolo3_darknet53(["a", "b", "c"], device="cpu", **kw)


@pytest.mark.parametrize("kw", [
    dict(), dict(k=3, k_join_type="max", k_join_pos="early"), dict(k=3, k_join_type="mean", k_join_pos="late"),
    dict(k=3, k_join_type="cat", k_join_pos="late", block_conv_type="3"), dict(k=3, k_join_type="max", k_join_pos="late", block_conv_type="21"),
    dict(k=3, corr_pos="early", corr_d=5), dict(k=2, corr_pos="late", corr_d=0)])
def test_set_storage_accepts_single_frames_and_every_window_variant(kw):
    net = _net(**kw)
    net.set_storage('bf16')
    assert net.storage == 'bf16'
    net.set_storage('fp32')
    with pytest.raises(ValueError):
        net.set_storage('fp16')
    # every stacked tensor keeps the copy kernels' 16-byte units when its bf16 channels go as 4-byte words
    from viddet_amd.model import PoolNode
    for n in net.nodes:
        if isinstance(n, PoolNode) and n.type == 2:
            assert net.tensors[n.src][0] % 8 == 0


def test_set_storage_refuses_the_out_of_scope_networks_by_name():
    from viddet_amd.model import yolo3_no_backbone
    nets = [_net(k=5, temporal=True, t_out=True), _net(k=5, temporal=True), yolo3_no_backbone(["a", "b"], device="cpu")]
    for net in nets:
        with pytest.raises(NotImplementedError, match="noback, temporal_out and temporal_side"):
            net.set_storage('bf16')
        assert getattr(net, 'storage', 'fp32') == 'fp32'
