"""CPU suite: the switch for the launches of an ICP iteration (include/tdv_hip.h: tdv_ctx_set_icp_launches, tdv_ctx_last_icp_launches).
The library exports both and lists them in ABI_SYMBOLS, refuses a null context and an unknown mode, and the Context methods map to them.
No compute entry point runs here; tests/test_gpu_icp_one_launch.py holds the kernel."""
import ctypes as C

import pytest

TDV_ERR_BAD_ARG = -2
SYMBOLS = ("tdv_ctx_set_icp_launches", "tdv_ctx_last_icp_launches")


def test_symbols(tdv):
    lib = tdv.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(tdv.ABI_SYMBOLS)


def test_null_context_and_bad_mode(tdv):
    lib = tdv.lib()
    for mode in (0, 1, 2, 3, -1):
        assert lib.tdv_ctx_set_icp_launches(None, mode) == TDV_ERR_BAD_ARG
    assert lib.tdv_ctx_last_icp_launches(None) == TDV_ERR_BAD_ARG


class FakeLib:
    """Records the calls the Context methods make."""

    def __init__(self):
        self.calls, self.last = [], 0

    def tdv_ctx_set_icp_launches(self, h, mode):
        self.calls.append(("set", h, mode))
        return 0 if 0 <= mode <= 2 else TDV_ERR_BAD_ARG

    def tdv_ctx_last_icp_launches(self, h):
        self.calls.append(("last", h))
        return self.last


def test_context_methods_map_to_the_symbols(tdv, monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(tdv, "lib", lambda: fake)
    ctx = tdv.Context.__new__(tdv.Context)          # no device: the methods only need the handle
    ctx._h = C.c_void_p(0x1234)
    assert tdv.Context.ICP_LAUNCHES == {"auto": 0, "two": 1, "one": 2}
    for name, mode in tdv.Context.ICP_LAUNCHES.items():
        ctx.set_icp_launches(name)
        assert fake.calls[-1] == ("set", ctx._h, mode)
        fake.last = mode
        assert ctx.last_icp_launches() == name and fake.calls[-1] == ("last", ctx._h)
    with pytest.raises(KeyError):
        ctx.set_icp_launches("three")
