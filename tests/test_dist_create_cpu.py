"""CPU: the argument checks of the three creators of a sharded state (qsim_dist_create,
qsim_dist_create_virtual, qsim_dist_create_hosted).  Every case is rejected before the first HIP
call, so it needs no device: the code is QSIM_ERR_INVALID_ARGUMENT, *out is left null and the
last-error text names the first check that fails, in the order the creators make them (null
arguments, world size, rank, qubit count)."""
import ctypes

import pytest

NULL_ARG = "null argument"
WORLD_POW2 = "world size must be a power of two"
WORLD_POS = "world size must be positive"
RANK = "rank out of range"
QUBITS = "Number of qubits out of range"
PER_RANK = "too few qubits per rank for this world size"
MAX_QUBITS_DIST = 36  # QSIM_MAX_QUBITS_DIST (include/qsim_hip.h)

# (n, world, rank, message): the cases every creator shares (rank is ignored by the virtual one)
SHARED = [
    (10, 3, 0, WORLD_POW2),
    (10, 0, 0, WORLD_POS),
    (0, 2, 0, QUBITS),
    (MAX_QUBITS_DIST + 1, 2, 0, QUBITS),
    (5, 8, 0, PER_RANK),  # n - g = 2 < g = 3
]
RANKED = [(10, 4, -1, RANK), (10, 4, 4, RANK)]
# two failing arguments at once: the earlier check answers
ORDER_RANKED = [(10, 3, -1, WORLD_POW2), (0, 4, 4, RANK)]


@pytest.fixture(scope="module")
def lib(qsim):
    from qsim_amd import _lib
    return _lib


def _callback(lib):
    return lib.qsim_dist_transport_fn(lambda ctx, posts, count: 0)


def _create(lib, which, n, world, rank, out, uid=True, fn=True):
    """Call creator `which` with device 0; uid / fn False pass a null id / callback."""
    keep = []
    if which == "rccl":
        buf = ctypes.create_string_buffer(128) if uid else None  # (never read: every case fails before)
        rc = lib.hip.qsim_dist_create(n, rank, world, buf, 0, out)
    elif which == "virtual":
        rc = lib.hip.qsim_dist_create_virtual(n, world, 0, out)
    else:
        cb = _callback(lib) if fn else lib.qsim_dist_transport_fn()
        keep.append(cb)
        rc = lib.hip.qsim_dist_create_hosted(n, rank, world, 0, cb, None, out)
    return rc, lib.hip.qsim_last_error().decode()


def _rejected(lib, which, n, world, rank, message, **kw):
    out = ctypes.c_void_p(0xdead)  # (a creator that gets as far as its checks clears it first)
    rc, msg = _create(lib, which, n, world, rank, ctypes.byref(out), **kw)
    assert rc == lib.QSIM_ERR_INVALID_ARGUMENT, (which, n, world, rank, rc, msg)
    assert msg == message, (which, n, world, rank, msg)
    assert not out.value, (which, n, world, rank)


@pytest.mark.parametrize("which", ["rccl", "virtual", "hosted"])
def test_null_out(lib, which):
    rc, msg = _create(lib, which, 10, 2, 0, None)
    assert rc == lib.QSIM_ERR_INVALID_ARGUMENT and msg == NULL_ARG, (rc, msg)
    # ... and before the world size is looked at
    rc, msg = _create(lib, which, 10, 3, 0, None)
    assert rc == lib.QSIM_ERR_INVALID_ARGUMENT and msg == NULL_ARG, (rc, msg)


@pytest.mark.parametrize("which", ["rccl", "virtual", "hosted"])
@pytest.mark.parametrize("n,world,rank,message", SHARED)
def test_shared_checks(lib, which, n, world, rank, message):
    _rejected(lib, which, n, world, rank, message)


@pytest.mark.parametrize("which", ["rccl", "hosted"])
@pytest.mark.parametrize("n,world,rank,message", RANKED + ORDER_RANKED)
def test_rank_checks(lib, which, n, world, rank, message):
    _rejected(lib, which, n, world, rank, message)


def test_null_id(lib):
    # (the null check comes first and leaves *out as it was)
    out = ctypes.c_void_p(0)
    rc, msg = _create(lib, "rccl", 10, 2, 0, ctypes.byref(out), uid=False)
    assert rc == lib.QSIM_ERR_INVALID_ARGUMENT and msg == NULL_ARG and not out.value, (rc, msg)
    rc, msg = _create(lib, "rccl", 10, 3, 0, ctypes.byref(out), uid=False)
    assert rc == lib.QSIM_ERR_INVALID_ARGUMENT and msg == NULL_ARG and not out.value, (rc, msg)


def test_null_callback(lib):
    out = ctypes.c_void_p(0)
    rc, msg = _create(lib, "hosted", 10, 2, 0, ctypes.byref(out), fn=False)
    assert rc == lib.QSIM_ERR_INVALID_ARGUMENT and msg == NULL_ARG and not out.value, (rc, msg)
    rc, msg = _create(lib, "hosted", 10, 3, 0, ctypes.byref(out), fn=False)
    assert rc == lib.QSIM_ERR_INVALID_ARGUMENT and msg == NULL_ARG and not out.value, (rc, msg)
