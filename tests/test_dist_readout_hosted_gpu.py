"""GPU: the sharded readout with one process per rank on the box's single GPU (host-staged
transport, tests/dist_readout_hosted.py): the vector all-reduces, the broadcast of the uniforms,
the 8 B / amplitude gather and the per-rank chunk maps of the multi-rank path.  Every rank must
report the same shots and the same measurement; the shots must match the oracle up to rounding
ties (tests/test_sampling_gpu.py's proof) and the measured state the oracle's collapse at 1e-12.
"""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _assert_tie_only(probs, u, got, exp):
    seq = np.add.accumulate(probs)  # sequential left-to-right, == std::partial_sum
    bad = np.nonzero(got != exp)[0]
    for i in bad:
        a, b = int(min(got[i], exp[i])), int(max(got[i], exp[i]))
        assert b - a == 1 or np.all(probs[a + 1:b] == 0.0), \
            f"shot {i}: indices {got[i]} vs {exp[i]} are not adjacent steps"
        k = a
        exact = math.fsum(probs[:k + 1])
        lo, hi = min(seq[k], exact), max(seq[k], exact)
        tol = 4 * np.spacing(u[i])
        assert lo - tol <= u[i] <= hi + tol, \
            f"shot {i}: u={u[i]!r} is not between C_seq={seq[k]!r} and C_exact={exact!r} at {k}"
    return len(bad)


def _ports(k):
    socks, ports = [], []
    for _ in range(k):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        socks.append(s)
        ports.append(s.getsockname()[1])
    for s in socks:
        s.close()
    return ports


@pytest.mark.subprocess  # started before this process initialises the GPU (pool rule)
@pytest.mark.parametrize("world,n", [(4, 16), (8, 10)])
def test_rank_processes_sample_and_measure(qsim, oracle, tmp_path, world, n):
    sys.path.insert(0, HERE)
    import dist_readout_hosted as helper
    ports = _ports(world)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "dist_readout_hosted.py"), str(r),
                               str(world), ",".join(map(str, ports)), str(n), str(tmp_path)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=100)
            outs.append(out.decode(errors="replace")[-3000:])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{outs[r]}"
    recs = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(world)]
    g = oracle.gates_of(helper.circuit(qsim, n))
    ref = oracle.run_cpu(n, g + g)
    probs = np.abs(ref) ** 2
    L = n - (world.bit_length() - 1)
    c = min(12, L)
    # the case starts with a chunk qubit on a rank position: the localization remap ran, on every rank alike
    assert any(recs[0]["perm_before"][q] >= L for q in range(c))
    assert all(recs[0]["perm_after"][q] < L for q in range(c))
    for rec in recs:
        for key in ("shots", "drawn", "perm_before", "perm_after", "bit", "result", "again"):
            assert rec[key] == recs[0][key], (key, rec["rank"])
        assert abs(rec["total"] - 1.0) < 1e-12
        assert rec["p0"] == recs[0]["p0"]
    u = helper.uniforms(n)
    got = np.array(recs[0]["shots"], dtype=np.int64)
    assert got[-1] == 1 << n
    _assert_tie_only(probs, u, got, oracle.sample_cpu(n, ref, u))
    drawn = np.array(recs[0]["drawn"])
    assert np.all(probs[drawn] > 0)
    np.testing.assert_allclose(np.load(tmp_path / "probs.npy"), probs, atol=1e-12, rtol=0)
    np.testing.assert_allclose(np.load(tmp_path / "state.npy"), ref, atol=1e-12, rtol=0)
    bit = recs[0]["bit"]
    assert recs[0]["perm_after"][bit] >= L                      # a rank position
    sel0 = ((np.arange(1 << n) >> bit) & 1) == 0
    p0 = float(probs[sel0].sum())
    assert abs(recs[0]["p0"] - p0) < 1e-12
    assert abs(p0 - helper.MEASURE_UNIFORM) > 1e-9              # (the outcome is not a rounding matter)
    result = 0 if helper.MEASURE_UNIFORM < p0 else 1
    assert recs[0]["result"] == result and recs[0]["again"] == result
    keep = sel0 if result == 0 else ~sel0
    want = np.where(keep, ref, 0.0) / math.sqrt(p0 if result == 0 else 1.0 - p0)
    np.testing.assert_allclose(np.load(tmp_path / "measured.npy"), want, atol=1e-12, rtol=0)
