"""Per-channel fine-tune NCO of the many-channel DDC: the host side of its C ABI, without a GPU.

  * sddc_ddc_set_channel_fine_tune and sddc_ddc_channel_tuning are exported and bound;
  * sddc_ddc_channel_tuning restates sddc_ddc_set_freq_offset (fft_mt_r2iq.cpp:101-109) without a
    handle: the same tune bin and the bit-same float residual, for every d;
  * argument checks of sddc_ddc_set_channel_fine_tune (a CPU handle has no many-channel path).
The GPU behaviour is in tests/test_gpu_channel_nco.py.
"""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest

NEW = ("sddc_ddc_set_channel_fine_tune", "sddc_ddc_channel_tuning")
OFFSETS = [0.0, 1.0 / 4096, 0.1234, 0.5, 0.99999, 1.25]   # the last one outside [0, 1)
ERR_ARG, ERR_STATE = -1, -4


@pytest.fixture()
def cpu_handle(ddc_lib):
    from extio_sddc_amd import DEVICE_CPU
    h = ctypes.c_void_p()
    assert ddc_lib.sddc_ddc_create(1.0, DEVICE_CPU, ctypes.byref(h)) == 0, ddc_lib.sddc_ddc_last_error()
    yield h
    ddc_lib.sddc_ddc_destroy(h)


def test_new_symbols_exported_and_bound(ddc_lib):
    from extio_sddc_amd._lib import LIB_PATH, SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (sddc_ddc_\w+)", out))
    for s in NEW:
        assert s in exported, s
        assert s in SIGNATURES, s
        assert hasattr(ddc_lib, s)
    assert ddc_lib.sddc_ddc_abi_version() == 3   # new symbols only


@pytest.mark.parametrize("d", range(7))
def test_channel_tuning_restates_set_freq_offset(ddc_lib, cpu_handle, d):
    assert ddc_lib.sddc_ddc_set_decimation(cpu_handle, d) == 0
    for off in OFFSETS:
        want_fc = np.float32(ddc_lib.sddc_ddc_set_freq_offset(cpu_handle, off))
        want_tb = ddc_lib.sddc_ddc_get_tunebin(cpu_handle)
        tb, fc = ctypes.c_int(-1), ctypes.c_float(np.nan)
        assert ddc_lib.sddc_ddc_channel_tuning(off, d, ctypes.byref(tb), ctypes.byref(fc)) == 0
        assert tb.value == want_tb, (off, d)
        assert np.float32(fc.value).view(np.uint32) == want_fc.view(np.uint32), (off, d)
    assert 0 <= tb.value <= 4092 and tb.value % 4 == 0   # the offset outside [0, 1) is clamped


def test_channel_tuning_python_helper(ddc_lib, cpu_handle):
    from extio_sddc_amd import channel_tuning
    d = 4
    tbs, fcs = channel_tuning(OFFSETS, d)
    assert tbs.dtype == np.int32 and fcs.dtype == np.float32 and tbs.shape == fcs.shape == (len(OFFSETS),)
    assert ddc_lib.sddc_ddc_set_decimation(cpu_handle, d) == 0
    for off, tb, fc in zip(OFFSETS, tbs, fcs):
        want = np.float32(ddc_lib.sddc_ddc_set_freq_offset(cpu_handle, off))
        assert (tb, fc.view(np.uint32)) == (ddc_lib.sddc_ddc_get_tunebin(cpu_handle), want.view(np.uint32))


def test_channel_tuning_argument_checks(ddc_lib):
    tb, fc = ctypes.c_int(0), ctypes.c_float(0.0)
    assert ddc_lib.sddc_ddc_channel_tuning(float("nan"), 0, ctypes.byref(tb), ctypes.byref(fc)) == ERR_ARG
    assert ddc_lib.sddc_ddc_channel_tuning(0.25, 7, ctypes.byref(tb), ctypes.byref(fc)) == ERR_ARG
    assert ddc_lib.sddc_ddc_channel_tuning(0.25, 0, None, ctypes.byref(fc)) == ERR_ARG


def test_set_channel_fine_tune_argument_checks(ddc_lib, cpu_handle):
    f = ddc_lib.sddc_ddc_set_channel_fine_tune
    ok = np.array([0.0, 0.01, -0.02], np.float32)
    assert f(None, ok.ctypes.data, ok.size) == ERR_ARG                      # null handle
    bad = np.array([0.0, np.nan, 0.01], np.float32)
    assert f(cpu_handle, bad.ctypes.data, bad.size) == ERR_ARG              # NaN
    assert b"channel 1" in ddc_lib.sddc_ddc_last_error()
    inf = np.array([np.inf], np.float32)
    assert f(cpu_handle, inf.ctypes.data, 1) == ERR_ARG
    many = np.zeros(1025, np.float32)
    assert f(cpu_handle, many.ctypes.data, 1025) == ERR_ARG                 # nch outside 0..1024
    assert f(cpu_handle, ok.ctypes.data, -1) == ERR_ARG
    assert f(cpu_handle, ok.ctypes.data, ok.size) == ERR_STATE              # a CPU handle
    assert f(cpu_handle, None, 0) == ERR_STATE


def test_python_wrapper_raises_on_cpu_handle(ddc_lib):
    from extio_sddc_amd import DEVICE_CPU, DDCError, R2iq
    with R2iq(gain=1.0, device=DEVICE_CPU) as r:
        with pytest.raises(DDCError) as e:
            r.setChannelFineTune([0.01, 0.02])
        assert e.value.code == ERR_STATE
        with pytest.raises(DDCError) as e:
            r.setChannelFineTune([0.01, float("nan")])
        assert e.value.code == ERR_ARG
