"""CPU suite: the argument rules of tdv_ctx_workspace_fill (include/tdv_hip.h), the test aid tests/test_gpu_ctx_state.py poisons a context
with.  Without a device there is no ctx: a NULL one is refused whatever the byte; the byte range on a real ctx is held in the GPU module."""
import os

TDV_ERR_BAD_ARG = -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_listed_and_documented(tdv):
    assert hasattr(tdv.lib(), "tdv_ctx_workspace_fill") and "tdv_ctx_workspace_fill" in tdv.ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "tdv_hip.h")).read()
    assert "int tdv_ctx_workspace_fill(tdv_ctx* ctx, int byte);" in header
    doc = header[:header.index("int tdv_ctx_workspace_fill(")].rsplit("/*", 1)[1]
    assert "Test aid" in doc and "NOT touched" in doc and "invariant" in doc


def test_null_ctx_is_refused_for_every_byte(tdv):
    lib = tdv.lib()
    for byte in (0, 1, 0x7F, 0xFF, -1, 256, -(1 << 31), (1 << 31) - 1):
        assert lib.tdv_ctx_workspace_fill(None, byte) == TDV_ERR_BAD_ARG, byte


def test_python_wrappers_exist(tdv):
    assert callable(tdv.Context.workspace_fill) and callable(tdv.Context.set_stream)


def test_last_voxel_batch_redone_is_exported_listed_and_refuses_a_null_ctx(tdv):
    assert hasattr(tdv.lib(), "tdv_ctx_last_voxel_batch_redone") and "tdv_ctx_last_voxel_batch_redone" in tdv.ABI_SYMBOLS
    assert "int tdv_ctx_last_voxel_batch_redone(tdv_ctx* ctx);" in open(os.path.join(ROOT, "include", "tdv_hip.h")).read()
    assert tdv.lib().tdv_ctx_last_voxel_batch_redone(None) == TDV_ERR_BAD_ARG and callable(tdv.Context.last_voxel_batch_redone)
