"""Host-side pieces of the batched overlap matrices (no GPU): qsim_batch_overlap_plan through
qsim_amd.plan.batch_overlap_plan — the tile counts of the self and the cross case, the partial
scratch, the kernel choice, the plan's dependence on the shapes alone — the argument errors and the
ctypes signatures."""
import ctypes

import pytest

TILE = 64
TILE_BYTES = TILE * TILE * 16


def _tiles(b):
    return (b + TILE - 1) // TILE


@pytest.mark.parametrize("n", [1, 5, 12, 16, 20])
@pytest.mark.parametrize("B", [1, 2, 17, 64, 65, 256, 1000])
def test_self_plan(qsim, n, B):
    from qsim_amd import plan
    info = plan.batch_overlap_plan(n, B)
    T = _tiles(B)
    assert info["row_tiles"] == info["col_tiles"] == T
    assert info["tiles"] == T * (T + 1) // 2
    assert info["chunks"] >= 1 and (1 << n) % info["chunks"] == 0
    assert info["scratch_bytes"] == info["chunks"] * info["tiles"] * TILE_BYTES
    assert info["mfma"] == (B > 1)


@pytest.mark.parametrize("n", [2, 12, 20])
@pytest.mark.parametrize("Ba,Bb", [(17, 5), (3, 33), (16, 16), (65, 129), (300, 1), (1, 300)])
def test_cross_plan(qsim, n, Ba, Bb):
    from qsim_amd import plan
    info = plan.batch_overlap_plan(n, Ba, Bb)
    assert (info["row_tiles"], info["col_tiles"]) == (_tiles(Ba), _tiles(Bb))
    assert info["tiles"] == _tiles(Ba) * _tiles(Bb)
    assert info["scratch_bytes"] == info["chunks"] * info["tiles"] * TILE_BYTES
    assert info["mfma"] == (Bb > 1), "one column is a GEMV: the FMA kernel"


def test_chunks(qsim):
    """Few tiles of a long K are cut into chunks (a chunk keeps at least 256 k); many tiles are not."""
    from qsim_amd import plan
    assert plan.batch_overlap_plan(1, 48)["chunks"] == 1
    assert plan.batch_overlap_plan(8, 48)["chunks"] == 1
    assert plan.batch_overlap_plan(12, 20)["chunks"] > 1
    assert plan.batch_overlap_plan(12, 20, 1)["chunks"] > 1
    assert plan.batch_overlap_plan(20, 16)["chunks"] > plan.batch_overlap_plan(12, 16)["chunks"]
    few, many = plan.batch_overlap_plan(16, 64), plan.batch_overlap_plan(16, 4096)
    assert few["chunks"] > many["chunks"] == 1
    for n, B in ((12, 20), (16, 256), (20, 16)):
        info = plan.batch_overlap_plan(n, B)
        assert (1 << n) // info["chunks"] >= 256


def test_scratch_needs_both_words(qsim):
    from qsim_amd import plan
    info = plan.batch_overlap_plan(1, 1 << 16)
    T = (1 << 16) // TILE
    assert info["tiles"] == T * (T + 1) // 2 and info["chunks"] == 1
    assert info["scratch_bytes"] == info["tiles"] * TILE_BYTES > 1 << 32


def test_plan_depends_on_the_arguments_alone(qsim, monkeypatch):
    """The kernel choice follows QSIM_OVERLAP_MFMA; the tiles, the chunks and the scratch do not,
    and repeated calls agree."""
    from qsim_amd import plan
    shapes = [(12, 20, None), (16, 256, None), (12, 17, 5), (20, 16, 1)]
    base = [plan.batch_overlap_plan(*s) for s in shapes]
    assert base == [plan.batch_overlap_plan(*s) for s in shapes]
    monkeypatch.setenv("QSIM_OVERLAP_MFMA", "0")
    off = [plan.batch_overlap_plan(*s) for s in shapes]
    assert not any(i["mfma"] for i in off)
    for a, b in zip(base, off):
        assert {k: v for k, v in a.items() if k != "mfma"} == {k: v for k, v in b.items() if k != "mfma"}


def test_errors(qsim):
    from qsim_amd import _lib, plan
    f = _lib.hip.qsim_batch_overlap_plan
    info = (ctypes.c_int32 * 8)()
    assert f(10, 3, 3, 1, info) == _lib.QSIM_OK and info[7] == 0
    assert f(10, 3, 4, 0, info) == _lib.QSIM_OK
    assert f(10, 3, 4, 1, info) == _lib.QSIM_ERR_INVALID_ARGUMENT  # self: one batch size
    assert f(0, 3, 3, 1, info) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(31, 3, 3, 1, info) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(10, 0, 3, 0, info) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(10, 3, 0, 0, info) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert f(10, 3, 3, 1, None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        plan.batch_overlap_plan(10, 0)


def test_signatures(qsim):
    from qsim_amd import _lib
    P, D = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
    assert _lib.hip.qsim_batch_overlaps.argtypes == [P, P, D]
    assert _lib.hip.qsim_batch_state_overlaps.argtypes == [P, P, D]
    assert _lib.hip.qsim_batch_overlap_plan.argtypes == [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int32)]
    for name in ("qsim_batch_overlaps", "qsim_batch_state_overlaps", "qsim_batch_overlap_plan"):
        assert getattr(_lib.hip, name).restype == ctypes.c_int
    for name in ("overlapMatrix", "kernelMatrix", "overlapsWith"):
        assert callable(getattr(qsim.BatchedSimulator, name))
    # null handles and a null result are refused before anything touches a device
    assert _lib.hip.qsim_batch_overlaps(None, None, None) == _lib.QSIM_ERR_INVALID_ARGUMENT
    assert _lib.hip.qsim_batch_state_overlaps(None, None, None) == _lib.QSIM_ERR_INVALID_ARGUMENT


def test_abi_version_unchanged(qsim):
    from qsim_amd import _lib
    assert _lib.hip.qsim_abi_version() == 2
