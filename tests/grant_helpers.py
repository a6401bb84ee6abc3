"""What the tests of the PDSCH grant calls (test_gpu_chan.py, test_gpu_txdiv.py, test_gpu_spmux.py, test_gpu_pdsch_csi.py, test_gpu_pdsch_rx_frame.py) and
tools/measure/csi_time.py build their arguments with: the library and its ctypes mirror, plane arrays, soft buffers of the reference's layout."""
import ctypes as C

import numpy as np

SB = 18600  # SRSRAN_HIP_SOFTBUFFER_CB_SIZE: entries of a soft-buffer row


def _lib():
    import srslte_amd as S
    from srslte_amd import capi

    return S.lib(), capi


def _planes(capi, arrs):
    return capi.PlaneArray(*[a.ctypes.data for a in arrs])


def _matrix(capi, h):
    """h [ports][nrx][n] -> cf_t* ce[port][rx]"""
    return capi.PlaneMatrix(*[_planes(capi, [h[k][r] for r in range(h.shape[1])]) for k in range(h.shape[0])])


def _rx_softbuffer(capi, max_cb, dt):
    rows = [np.zeros(SB, dt) for _ in range(max_cb)]
    keep = [np.zeros(SB // 8, np.uint8) for _ in range(max_cb)]
    flags = np.zeros(max_cb, np.bool_)
    sb = capi.SoftbufferRx(max_cb, SB, (C.c_void_p * max_cb)(*[r.ctypes.data for r in rows]), (C.c_void_p * max_cb)(*[k.ctypes.data for k in keep]),
                           flags.ctypes.data_as(C.POINTER(C.c_bool)), False)
    return sb, rows, keep, flags


def _tx_softbuffer(capi, max_cb):
    rows = [np.zeros(SB, np.uint8) for _ in range(max_cb)]
    return capi.SoftbufferTx(max_cb, SB, (C.c_void_p * max_cb)(*[r.ctypes.data for r in rows])), rows
