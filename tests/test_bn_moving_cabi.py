"""BatchNorm moving statistics, C ABI: the `_ex` finalize entry points reject a bad dspn_bn_moving block before any HIP
call (no GPU needed), and the builders refuse a fixed-statistics training graph."""
import ctypes

import pytest

from dspnet_amd import _lib
from dspnet_amd import functional as fn


def _calls():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)        # never dereferenced: every call below fails its checks first
    eps = ctypes.c_float(2e-5)

    def plain_f32(mv):
        return lib.dspn_bn_stats_ex_f32(p, 512, 8, eps, None, p, p, p, p, p, p, 1 << 20, mv, None)

    def plain_bf16(mv):
        return lib.dspn_bn_stats_ex_bf16(p, 512, 8, eps, None, p, p, p, p, p, p, 1 << 20, mv, None)

    def tiles(mv):
        return lib.dspn_bn_stats_from_tiles_ex_f32(p, 4, 128, 512, 8, eps, None, p, p, p, p, p, None, 0, None, None, None,
                                                   None, 0, mv, None)
    return {"bn_stats_ex_f32": plain_f32, "bn_stats_ex_bf16": plain_bf16, "bn_stats_from_tiles_ex": tiles}


def _block(mean=256, var=256, momentum=0.9, mode=fn.BN_TRACK, channels=0):
    return ctypes.byref(fn.BnMoving(mean, var, momentum, mode, channels))


@pytest.mark.parametrize("entry", ["bn_stats_ex_f32", "bn_stats_ex_bf16", "bn_stats_from_tiles_ex"])
def test_moving_block_validation_without_gpu(entry):
    call = _calls()[entry]
    lib = _lib.lib()
    for bad in (-0.1, 1.5, float("nan")):
        assert call(_block(momentum=bad)) == -1
        assert b"momentum must be in [0, 1]" in lib.dspn_last_error()
    for mean, var in ((None, 256), (256, None), (None, None)):
        assert call(_block(mean=mean, var=var)) == -1
        assert b"moving_mean and moving_var must not be NULL" in lib.dspn_last_error()
    for mode in (0, 3, -1):
        assert call(_block(mode=mode)) == -1
        assert b"DSPN_BN_TRACK or DSPN_BN_GLOBAL" in lib.dspn_last_error()
    assert call(_block(channels=9)) == -1 and b"channels must be in [0, C]" in lib.dspn_last_error()
    assert call(_block(channels=-1)) == -1 and b"channels must be in [0, C]" in lib.dspn_last_error()
    # a valid block gets as far as the checks of the plain entry point (NULL mean below / rows vs tiles)
    for momentum in (0.0, 1.0):
        for mode in (fn.BN_TRACK, fn.BN_GLOBAL):
            if entry == "bn_stats_from_tiles_ex":
                rc = lib.dspn_bn_stats_from_tiles_ex_f32(ctypes.c_void_p(256), 4, 128, 9999, 8, ctypes.c_float(2e-5), None,
                                                         ctypes.c_void_p(256), *([ctypes.c_void_p(256)] * 4), None, 0, None,
                                                         None, None, None, 0, _block(momentum=momentum, mode=mode), None)
                assert rc == -1 and b"bn_stats_from_tiles: bad argument" in lib.dspn_last_error()
            else:
                f = lib.dspn_bn_stats_ex_f32 if entry.endswith("f32") else lib.dspn_bn_stats_ex_bf16
                rc = f(ctypes.c_void_p(256), 512, 8, ctypes.c_float(2e-5), None, ctypes.c_void_p(256), None,
                       *([ctypes.c_void_p(256)] * 4), 1 << 20, _block(momentum=momentum, mode=mode), None)
                assert rc == -1 and b"bn_stats: null pointer" in lib.dspn_last_error()


def test_ex_with_null_block_is_the_plain_entry_point():
    """moving == NULL: the same checks (and the same launches) as the entry point without `_ex`"""
    lib = _lib.lib()
    p, eps = ctypes.c_void_p(256), ctypes.c_float(2e-5)
    assert lib.dspn_bn_stats_ex_f32(p, 512, 6, eps, None, p, p, p, p, p, p, 1 << 20, None, None) == -1
    assert b"multiple of 4" in lib.dspn_last_error()
    assert lib.dspn_bn_stats_ex_f32(p, 512, 8, eps, None, p, p, p, p, p, p, 16, None, None) == -2
    assert b"workspace too small" in lib.dspn_last_error()
    assert lib.dspn_bn_stats_from_tiles_ex_f32(p, 4, 128, 512, 8, eps, None, p, p, p, p, p, p, 0, None, None, None, None, 0,
                                               None, None) == -1
    assert b"go together" in lib.dspn_last_error()


@pytest.mark.parametrize("builder", ["get_multi_symbol_train", "get_det_symbol_train", "get_seg_symbol_train"])
def test_training_builders_reject_global_stats(builder):
    import torch
    from dspnet_amd.symbol import multitask_symbol_factory as f
    with pytest.raises(ValueError, match="use_global_stats"):
        getattr(f, builder)("resnet-50", 128, num_classes=8, batch_size=1, device=torch.device("cpu"), use_global_stats=True)
    with pytest.raises(ValueError, match="bn_mom"):
        getattr(f, builder)("resnet-50", 128, num_classes=8, batch_size=1, device=torch.device("cpu"), bn_mom=1.5)
