"""CPU suite: the batched ICP entry points (tdv_icp_batch_dev, tdv_refine_batch_dev) exist and refuse a null ctx before touching
any other argument.  No compute entry point runs here."""
import ctypes as C

TDV_ERR_BAD_ARG = -2


def test_null_ctx_is_a_bad_argument(tdv):
    lib = tdv.lib()
    off = (C.c_int * 2)(0, 0)
    T0 = (C.c_float * 16)(*[1.0 if i % 5 == 0 else 0.0 for i in range(16)])
    out = (tdv.IcpResultC * 1)()
    assert lib.tdv_icp_batch_dev(None, None, off, 1, None, None, 0, T0, C.c_float(0.01), 10, 1, 0, out) == TDV_ERR_BAD_ARG
    assert lib.tdv_icp_batch_dev(None, None, None, 0, None, None, 0, None, C.c_float(0.01), 10, 1, 0, None) == TDV_ERR_BAD_ARG
    prm = tdv.batch_params()
    res = (tdv.InstanceResultC * 1)()
    assert lib.tdv_refine_batch_dev(None, None, None, None, 1, C.byref(prm), T0, None, None, 0, res) == TDV_ERR_BAD_ARG
    assert lib.tdv_refine_batch_dev(None, None, None, None, 0, None, None, None, None, 0, None) == TDV_ERR_BAD_ARG
