"""Operand-class cases, class keys and checks for the density-matrix passes: csrc/hip/density.hip
lowers every gate into U on the row bit q + n and conj(U) on the column bit q, every channel into
controlled 2x2 and diagonal ops on that bit pair, and runs them through the pass kernels of
fused.hip and the generated kernels of jit.hip (tests/fused_cases.py pins those on the
state-vector gate set, which cannot produce the real 2x2, the real scales, the CX . diag . CX
triples or the conjugated column ops).

Helper module (no tests here), shared by tests/test_dm_pass_matrix_cpu.py,
tests/test_dm_pass_matrix_gpu.py and the child script tests/dm_pass_child.py.

  * `reference`: gates as U rho U^dag, channels in Kraus form, in plain numpy on the 2^n x 2^n
    matrix (2x2 definitions of pergate_cases; nothing from oracle/ or the engine); also returns the
    may-change mask.
  * `classes_of`: fused_cases.class_of plus the source gate type, the op's origin (gate row / gate
    column / sign / channel type), for channel ops the role pair (row bit, column bit) and for a
    CX . diag . CX triple the form Gen::xor_diag gives it.
  * `cases`, `required`, `generated_circuits`, `check`, `run_matrix`, `run_generated`: as in
    fused_cases; `run_relabeled`: the case as the second run under a first run's labels (with
    `search_relabeled`, cases chosen from the plans under those labels); `run_channels`: applyChannel.
"""
import math

import numpy as np

import fused_cases as fc
import pergate_cases as pc
from fused_cases import ANY, K_DIAG, K_M1, K_SWAP, S_GEN, S_X  # noqa: F401
from pergate_cases import X, Y, Z, H, S, T, SDAG, TDAG, RX, RY, RZ, CNOT, CZ, SWAP  # noqa: F401

TOL = pc.TOL
ONE_Q = list(range(X, RZ + 1))
DIAG_Q = [Z, S, T, SDAG, TDAG, RZ]
CH_NAMES = ["depolarizing", "amplitude damping", "phase damping", "bit flip", "phase flip", "bit-phase flip"]
REFERENCE_Y = 8  # QSIM_DM_REFERENCE_Y


# ------------------------------------------------------------------------------ settings
def settings(name, n, h=None, rb7=None, ctrl_out=1, env=None, anchor=True, relabeled=False):
    """One configuration (fused_cases.settings, n = qubits of rho: 2n index bits).  anchor (h = 7):
    every case starts with Z on anchor_qubits(n), see there."""
    return {"name": name, "n": n, "h": h, "rb7": rb7, "ctrl_out": ctrl_out, "env": dict(env or {}),
            "anchor": anchor and h == 7, "relabeled": relabeled}


apply_settings = fc.apply_settings
restore_settings = fc.restore_settings


def anchor_qubits(n):
    """plan_fused (QSIM_TILE_MIX) demotes a pass of a 13-bit plan to a 12-bit tile when the bits its
    ops need from r on number at most 12 - r for some run width r in 4..6.  Z on a qubit is exact,
    claims no register bit and needs the qubit's row and column bit.  Nine bits from 4 up fit no
    12-bit tile and, with bits 0..3, exactly fill a 13-bit one, so the cases stay on these qubits:
    n = 7: qubits 1..6 (bits 4, 5, 6 and 8..13); n = 8: qubits 3..7 (bits 4..7 and 11..15)."""
    return {7: [1, 2, 3, 4, 5, 6], 8: [3, 4, 5, 6, 7]}[n]


def shape(s):
    """(h, rb, r0) of the passes of 2n index bits (fused_cases.shape on the state of rho)."""
    return fc.shape(dict(s, n=2 * s["n"]))


NATURAL = [settings(f"n{n}", n) for n in range(3, 9)]
FORCED = ([settings(f"h{h}_n{(7 + h) // 2}", (7 + h) // 2, h=h) for h in range(6)] +
          [settings(f"h7rb{rb}_n{n}", n, h=7, rb7=rb) for n in (7, 8) for rb in (4, 3)] +
          [settings("h7mix_n7", 7, h=7, anchor=False)])
CTRL_OUT_OFF = [settings("n8_co0", 8, ctrl_out=0)]
IN_PROCESS = NATURAL + FORCED + CTRL_OUT_OFF
# Generated kernels (set_jit(2, 0)): the staged configurations (jit.hip specialises passes of h >= 4
# only), each pass shape once: h4_n5 is n5 again; of the four anchored h = 7 configurations each
# stage width and each size runs once (rb 4 at n = 7, rb 3 at n = 8), since every configuration costs
# a compile per circuit; n8_co0 plans like n8 without the tile-constant classes.
GENERATED = [c for c in NATURAL + FORCED[5:] if shape(c)[1] > 0 and c["name"] not in ("h7rb3_n7", "h7rb4_n8")]
# one hipRTC compile per circuit: fused_cases stays within 20 per configuration for about 90
# required patterns; here up to 190 patterns need a few more
MAX_GENERATED = 30
KNOBS = fc.KNOBS + ("QSIM_JIT_XOR_DIAG", "QSIM_DM_RELABEL_MIN_BITS", "QSIM_DM_RELABEL_TRIES")
# Knobs read once per process: each variant runs in a child (tests/dm_pass_child.py).  "jit": the
# generated kernels; "relabeled": the case runs second, under the labels of a first run.
CHILDREN = [
    [dict(settings("xor0_n7", 7, env={"QSIM_JIT_XOR_DIAG": 0}), jit=True),
     dict(settings("xor0_n6", 6, env={"QSIM_JIT_XOR_DIAG": 0}), jit=True)],
    [settings("rb4_n7", 7, env={"QSIM_TILE_RB": 4}), settings("rb4_n6", 6, env={"QSIM_TILE_RB": 4})],
    [settings("r0_4_n7", 7, env={"QSIM_TILE_R0": 4})],
    [settings("relabel_n8", 8, env={"QSIM_DM_RELABEL_MIN_BITS": 12}, relabeled=True),
     settings("relabel_n7", 7, env={"QSIM_DM_RELABEL_MIN_BITS": 12}, relabeled=True)],
    [dict(settings("relabel_jit_n8", 8, env={"QSIM_DM_RELABEL_MIN_BITS": 12}, relabeled=True), jit=True)],
]


# ------------------------------------------------------------------------------ reference
def _side(n, v, t, qs, p, row):
    """One gate on the row bits (U v) or on the column bits (conj(U) v = conj(U conj(v))) of the
    flattened matrix v[i * 2^n + j] = rho[i][j]."""
    if row:
        return pc.dense_apply(2 * n, v, t, [q + n for q in qs], p)
    out, may = pc.dense_apply(2 * n, np.conj(v), t, list(qs), p)
    return np.conj(out), may


def _kraus(n, v, q, ks):
    """sum_k K rho K^dag for 2x2 Kraus operators on qubit q: K on the row bit, conj(K) on the
    column bit."""
    out = np.zeros_like(v)
    for k in ks:
        a, _ = pc.dense_matrix1q(2 * n, v, q + n, k)
        b, _ = pc.dense_matrix1q(2 * n, np.conj(a), q, k)
        out += np.conj(b)
    return out


_I2, _X2, _Z2 = np.eye(2), np.array([[0.0, 1.0], [1.0, 0.0]]), np.diag([1.0, -1.0])


def kraus_of(t, p):
    """The Kraus operators of channel type t as this project defines it."""
    flip = lambda prob, m: [math.sqrt(1.0 - prob) * _I2, math.sqrt(prob) * m]
    if t == 0:  # off-diagonal x (1 - 4p/3), diagonal kept: a phase flip with probability 2p/3
        return flip(2.0 * p / 3.0, _Z2)
    if t == 1:
        return [np.diag([1.0, math.sqrt(1.0 - p)]), np.array([[0.0, math.sqrt(p)], [0.0, 0.0]])]
    if t == 2:
        return [np.diag([1.0, math.sqrt(1.0 - p)]), np.diag([0.0, math.sqrt(p)])]
    if t == 3:
        return flip(p, _X2)
    if t in (4, 5):  # bit-phase flip is the phase-flip channel here (density.hip)
        return flip(p, _Z2)
    raise ValueError(t)


def channel(n, rho, t, q, p):
    """(rho after the channel, may-change mask) on the 2^n x 2^n matrix."""
    v = np.asarray(rho, np.complex128).reshape(-1)
    idx = np.arange(1 << (2 * n), dtype=np.int64)
    differ = ((idx >> q) & 1) != ((idx >> (q + n)) & 1)
    may = differ if t in (0, 2, 4, 5) else np.ones_like(differ)
    return _kraus(n, v, q, kraus_of(t, p)).reshape(1 << n, 1 << n), may.reshape(1 << n, 1 << n)


def reference(n, rho, gates, channels=(), reference_y=False):
    """(rho, may_change) of DensityMatrixSimulator.run: every gate as U rho U^dag (negated after a
    Y with reference_y), then per qubit of the gate every channel (type, qubit or -1, p) that applies,
    in model order (the order of density.hip dm_lower)."""
    d = 1 << n
    v = np.asarray(rho, np.complex128).reshape(-1).copy()
    may = np.zeros(d * d, bool)
    for t, qs, p in gates:
        v, m1 = _side(n, v, t, qs, p, True)
        v, m2 = _side(n, v, t, qs, p, False)
        may |= m1 | m2
        if reference_y and t == Y:
            v = -v
            may[:] = True
        for q in qs:
            for ct, cq, cp in channels:
                if cq < 0 or cq == q:
                    out, m = channel(n, v.reshape(d, d), ct, q, cp)
                    v = out.reshape(-1)
                    may |= m.reshape(-1)
    return v.reshape(d, d), may.reshape(d, d)


def dense_rho(n, seed):
    """Dense complex Gaussian 2^n x 2^n matrix: not Hermitian, not positive, not of trace one (every
    op is linear; a general matrix separates row from column and U from conj(U))."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(1 << n, 1 << n)) + 1j * rng.normal(size=(1 << n, 1 << n))
    assert np.all(a.real != 0.0) and np.all(a.imag != 0.0)
    return a


def circuit_of(qsim, n, gates):
    return fc.circuit_of(qsim, n, gates)


def noise_of(qsim, channels):
    nm = qsim.NoiseModel()
    adders = [nm.addDepolarizing, nm.addAmplitudeDamping, nm.addPhaseDamping, nm.addBitFlip,
              nm.addPhaseFlip, nm.addBitPhaseFlip]
    for t, q, p in channels:
        adders[t](p) if q < 0 else adders[t]([q], p)
    return nm


def plan_info(qsim, n, case, perm=None):
    from qsim_amd import plan
    _, gates, channels, ref_y = case
    return plan.dm_plan_stage_info(circuit_of(qsim, n, gates), channels, 1 | (REFERENCE_Y if ref_y else 0), perm)


def jit_source(qsim, n, case):
    """The generated kernel source of the case's plan under identity labels (qsim_dm_jit_source)."""
    import ctypes
    from qsim_amd import _lib
    _, gates, channels, ref_y = case
    g, ng = circuit_of(qsim, n, gates).to_abi()
    arr = (_lib.qsim_noise_channel * max(1, len(channels)))()
    for i, (t, q, p) in enumerate(channels):
        arr[i].type, arr[i].qubit, arr[i].probability = t, q, p
    flags, size = 1 | (REFERENCE_Y if ref_y else 0), ctypes.c_size_t()
    _lib.check(_lib.hip.qsim_dm_jit_source(n, g, ng, arr, len(channels), flags, None, 0, ctypes.byref(size)))
    buf = ctypes.create_string_buffer(size.value + 1)
    _lib.check(_lib.hip.qsim_dm_jit_source(n, g, ng, arr, len(channels), flags, buf, size.value + 1,
                                           ctypes.byref(size)))
    return buf.value.decode()


def xor_factor_lines(src):
    """The per-lane factor pairs `const double f<i> = c<j> ? g : 1.0, f<k> = ...` that only
    Gen::xor_diag's thread-bit / tile-constant branch emits."""
    return [ln for ln in src.splitlines() if ln.lstrip().startswith("const double f") and "? 1.0 :" in ln]


# ------------------------------------------------------------------------------ class keys
def _role(bit, ps, stage):
    """Role of physical index bit `bit` in stage `stage` of pass record ps: reg / thr / out (staged),
    lane / high (unstaged), "" (per-gate)."""
    if ps["single"]:
        return ""
    tb = bit if bit < ps["r0"] else (ps["r0"] + ps["hpos"].index(bit) if bit in ps["hpos"] else -1)
    if ps["rb"] == 0:
        return "lane" if 0 <= tb < 6 else "high"
    if tb < 0:
        return "out"
    return "reg" if (ps["stage_bits"][stage] >> tb) & 1 else "thr"


def _xor_form(a, b, c):
    """The form Gen::xor_diag (jit.hip) gives the ops a, b, c of one stage, adjacent in this order;
    mirrors its conditions: a, c the same X on a register bit under exactly one control bit, b a
    real one-sided general diagonal on that register bit without controls."""
    one_bit = lambda m: m != 0 and m & (m - 1) == 0
    ctl = lambda r: (r["cm_reg"], r["cm_thr"], r["cm_out"])
    nc = sum(m != 0 for m in ctl(a))
    if a["kind"] != K_M1 or a["sub"] != S_X or a["p0"] < 0 or nc != 1 or not one_bit(a["cm_reg"] | a["cm_thr"] | a["cm_out"]):
        return "split"
    if (c["kind"], c["sub"], c["p0"]) != (a["kind"], a["sub"], a["p0"]) or ctl(c) != ctl(a):
        return "split"
    if b["kind"] != K_DIAG or b["sub"] != S_GEN or b["p0"] != a["p0"] or not b["d0_one"] or any(ctl(b)):
        return "split"  # (b.m[3] == 0: every channel scale is real)
    return "xor_reg" if a["cm_reg"] else "xor_thr" if a["cm_thr"] else "xor_out"


def classes_of(info, n, gates, perm=None):
    """The class keys of a plan's op records:
    fused_cases.class_of + (gate type, origin, role pair, xor form).
      gate type  name of the source gate for a gate op, "" for a channel op
      origin     row / col / sign / ch0..ch5
      role pair  channel ops: (role of the row bit, role of the column bit) of the channel's qubit
                 in the op's stage; the op's own target on a register bit reads p<k>
      xor form   ops of a CX . diag . CX channel (types 0, 2, 4, 5): xor_reg / xor_thr / xor_out when
                 the three are adjacent in one stage and Gen::xor_diag collapses them, else split
    """
    perm = list(range(2 * n)) if perm is None else list(perm)
    recs, passes = info["ops"], info["passes"]
    xor = {}
    triples = {}
    for i, r in enumerate(recs):
        if r["origin"] in ("ch0", "ch2", "ch4", "ch5"):
            triples.setdefault((r["src"], r["qubit"], r["origin"]), []).append(i)
    for idx in triples.values():
        for k in range(0, len(idx) - 2, 3):
            ia, ib, ic = sorted(idx[k:k + 3], key=lambda i: recs[i]["seq"])
            a, b, c = recs[ia], recs[ib], recs[ic]
            staged = not passes[a["pass"]]["single"] and passes[a["pass"]]["rb"] > 0
            together = (ib, ic) == (ia + 1, ia + 2) and len({(r["pass"], r["stage"]) for r in (a, b, c)}) == 1
            form = _xor_form(a, b, c) if staged and together else "split"
            for i in (ia, ib, ic):
                xor[i] = form
    out = set()
    origin, gtype = "", ""
    for i, r in enumerate(recs):
        ps = passes[r["pass"]]
        if r["origin"]:  # (the second and third op of a lowered SWAP keep the first one's)
            origin = r["origin"]
            gtype = pc.NAMES[gates[r["src"]][0]] if origin in ("row", "col", "sign") else ""
        pair = ()
        if origin.startswith("ch"):
            rbit, cbit = perm[r["qubit"] + n], perm[r["qubit"]]
            roles = []
            for bit in (rbit, cbit):
                role = _role(bit, ps, r["stage"])
                if role == "reg" and r["p0"] >= 0 and not ps["single"]:
                    tb = bit if bit < ps["r0"] else ps["r0"] + ps["hpos"].index(bit)
                    if tb == r["b0"]:
                        role = f"p{r['p0']}"
                roles.append(role)
            pair = tuple(roles)
        out.add(fc.class_of(r, ps) + (gtype, origin, pair, xor.get(i, "")))
    return out


def matches(pattern, key):
    """fused_cases.matches; a set in the pattern matches any of its members."""
    return all(p is ANY or (k in p if isinstance(p, (set, frozenset)) else p == k) for p, k in zip(pattern, key))


def missing(required_patterns, hit):
    return [p for p in required_patterns if not any(matches(p, k) for k in hit)]


def _pat(fam=ANY, pos=ANY, arm=ANY, tgt=ANY, ctl=ANY, d0=ANY, r0=ANY, gate=ANY, origin=ANY, pair=ANY, xor=ANY):
    return (fam, pos, arm, tgt, ctl, d0, r0, gate, origin, pair, xor)


def required(s):
    """The class patterns configuration `s` must hit, from the branches of stage_op / stage_m1_arm /
    stage_diag and k_fused_tile (fused.hip), Gen::op_body / diag1 / scale / xor_diag (jit.hip) and the
    lowering (density.hip dm_col, dm_row, dm_channel).

    Every configuration: each gate type on the row and on the column side (dm_col's swaps S <-> Sdag,
    T <-> Tdag, conj(Y) as a general 2x2, negated imaginary parts of Rx / Ry / Rz); the sign op of
    QSIM_DM_REFERENCE_Y; each channel type; amplitude damping's controlled real 2x2 and its two-sided
    real diagonal, bit flip's uncontrolled real 2x2.

    Staged: the 1-qubit gates on each register bit of a stage and, the diagonal ones, on a thread
    bit; CNOT and CZ controlled from reg / thr / out; for depolarizing (which stands for the shared
    `case 0/2/4/5` of dm_channel), amplitude damping and bit flip the CX with the row bit on every
    register bit crossed with the column bit in reg / thr / out; amplitude damping's real 2x2 on the
    column bit controlled from reg / thr / out; the xor forms and split; every stage position.
    Left out as unreachable:
      * `out` where every index bit is a tile bit (2n == 6 + h), with set_tile_ctrl_out(0), and in
        the anchored h = 7 configurations (the cases stay on the anchor's qubits, all in the tile);
      * the role pair (p0, reg) under identity labels: a stage numbers its register bits in ascending
        tile-bit order (fused.hip, `if ((sbits >> b) & 1u) fix[nf++] = b`), tile bits keep the order
        of the index bits, and the row bit q + n lies above the column bit q.  The relabeled
        configurations, where the bits move independently, are the ones that can reach it;
      * `out` for amplitude damping and bit flip, and a tile-constant control on amplitude
        damping's 2x2: their sequences hold a 2x2 on the column bit, and the row bit is the target
        of the ops before and after it, so either bit is outside the tile only where a pass boundary
        falls inside the channel.  For depolarizing one `out` class is required, not the cross with
        every register bit: the padding of a tile takes the low bits first, so the column bit is
        outside only in a pass full of other bits, whose register bits the case cannot also choose;
      * `split`: the three ops of a triple name the same two bits, so plan_stages defers all of
        them or none and keeps them adjacent in one stage; no case of any configuration plans
        otherwise.  classes_of still reports it, and the three-op emission runs in the child with
        QSIM_JIT_XOR_DIAG=0, which checks in the generated source that the knob took effect (no
        per-lane factor pairs there, xor_factor_lines; with the knob on every such circuit has them);
      * 2x2 targets on thread bits (plan_stages gives every 2x2 target a register bit).
    Unstaged (k_fused_tile): targets on lane and on high bits (h > 0), controls inside the tile; a
    per-gate step where an op needs more bits from 6 up than the tile has (h = 1 at n = 4)."""
    n = s["n"]
    h, rb, r0 = shape(s)
    one_q = [pc.NAMES[t] for t in ONE_Q]
    out = []
    for side in ("row", "col"):
        for g in one_q + ["CNOT", "CZ", "SWAP"]:
            out.append(_pat(gate=g, origin=side))
    out.append(_pat(origin="sign", d0=0))
    for t in range(6):
        out.append(_pat(origin=f"ch{t}"))
    if rb == 0:
        fam = f"tile{h}"
        tgts = ["lane"] + (["high"] if h > 0 else [])
        for side, tg in (("row", tgts[-1]), ("col", "lane")):  # (row bits are the high ones)
            for g in one_q:
                out.append(_pat(fam=fam, tgt=tg, gate=g, origin=side))
            out.append(_pat(fam=fam, arm="m1", ctl=("tile",), gate="CNOT", origin=side))
            out.append(_pat(fam=fam, arm="diag", ctl=("tile",), gate="CZ", origin=side))
            out.append(_pat(fam=fam, arm="swap", gate="SWAP", origin=side))
        for t in range(6):
            out.append(_pat(fam=fam, arm="m1", ctl=("tile",), origin=f"ch{t}"))    # the CX
        for t, g in ((0, 1), (2, 1), (4, 1), (5, 1), (1, 0)):
            out.append(_pat(fam=fam, arm="diag", ctl=(), d0=g, origin=f"ch{t}"))  # real scales
        out.append(_pat(fam=fam, arm="m1", ctl=("tile",), origin="ch1", pair={("lane", "lane"), ("high", "lane")}))
        out.append(_pat(fam=fam, arm="m1", ctl=(), origin="ch3"))
        if h == 1 and n == 4:
            out.append(_pat(fam="single"))
        return out
    fam = ("staged", h, rb)
    has_out = 2 * n > 6 + h and s["ctrl_out"] == 1 and not s["anchor"]
    ctl_roles = ["reg", "thr"] + (["out"] if has_out else [])
    regs = [f"p{p}" for p in range(rb)]
    diag_names = {pc.NAMES[t] for t in DIAG_Q}
    for side in ("row", "col"):
        for g in one_q:
            for p in regs:
                out.append(_pat(fam=fam, tgt=p, r0=r0, gate=g, origin=side))
            if g in diag_names:
                out.append(_pat(fam=fam, tgt={"thr_lo", "thr_hi"}, r0=r0, gate=g, origin=side))
        for c in ctl_roles:
            out.append(_pat(fam=fam, arm="swap", ctl=(c,), gate="CNOT", origin=side))
            out.append(_pat(fam=fam, arm="neg", ctl=(c,), gate="CZ", origin=side))
        out.append(_pat(fam=fam, arm="swap", gate="SWAP", origin=side))
    for t in (0, 1, 3):  # the CX of the channel: row bit on every register bit x column bit role
        for p in regs:
            for c in ("reg", "thr"):
                if (p, c) != ("p0", "reg"):
                    out.append(_pat(fam=fam, arm="swap", tgt=p, ctl=(c,), origin=f"ch{t}", pair=(p, c)))
    if has_out:
        out.append(_pat(fam=fam, arm="swap", ctl=("out",), origin="ch0"))
    for t, d0 in ((0, 1), (2, 1), (4, 1), (5, 1), (1, 0)):  # Gen::scale, real, one- and two-sided
        out.append(_pat(fam=fam, arm="phase", ctl=(), d0=d0, origin=f"ch{t}"))
    for c in ("reg", "thr"):  # amplitude damping: the real 2x2 on the column bit, controlled by the row bit
        out.append(_pat(fam=fam, arm="gen", ctl=(c,), origin="ch1"))
    for p in regs:            # bit flip: the real 2x2 without a control
        out.append(_pat(fam=fam, arm="gen", tgt=p, ctl=(), origin="ch3"))
    for form in ["xor_reg", "xor_thr"] + (["xor_out"] if has_out else []):
        out.append(_pat(fam=fam, xor=form))
    for pos in ("first", "middle", "last", "only"):
        out.append(_pat(fam=fam, pos=pos, origin={"row", "col"}))
        out.append(_pat(fam=fam, pos=pos, origin={f"ch{t}" for t in range(6)}))
    return out


def required_relabeled(s):
    """What a relabeled configuration must hit, from the plans under the state's own perm(): row
    and column bits move independently under the first run's labels, so a channel can have its
    column bit on a register bit of a first or last stage (high tile bits only) while its row bit is
    a thread bit -- under identity labels column bits are the low ones; and one xor form."""
    h, rb, _ = shape(s)
    chans = {f"ch{t}" for t in range(6)}
    return [_pat(fam=("staged", h, rb), pos={"first", "last"}, origin=chans,
                 pair={("thr", f"p{p}") for p in range(rb)} | {("thr", "reg")}),
            _pat(fam=("staged", h, rb), xor={"xor_reg", "xor_thr", "xor_out"})]


def search_cases(qsim, s, want, perm=None, tries=4000, seed=17, keep=2, channel_types=(1, 1, 3, 0)):
    """Seeded random search over the host planner: circuits of 2 to 6 gates on any qubits with one
    channel whose plan (under the labels perm) hits a pattern of `want` not hit before; at most
    `keep`.  Chosen from the plans alone, never from a result.  STEERED was filled this way from the
    patterns of required(s) the constructed cases miss."""
    n = s["n"]
    left = list(want)
    rng = np.random.default_rng(seed + n)
    types = ONE_Q + [CNOT, CZ, SWAP]
    out = []
    for _ in range(tries):
        if not left or len(out) >= keep:
            break
        gs = []
        for _ in range(int(rng.integers(2, 7))):
            t = int(rng.choice(types))
            qs = [int(x) for x in rng.choice(n, size=1 if t <= RZ else 2, replace=False)]
            gs.append((t, qs, fc._angle(rng) if t in (RX, RY, RZ) else 0.0))
        ct = int(rng.choice(channel_types))
        case = (f"searched{len(out)}", gs, [(ct, -1 if rng.integers(2) else int(rng.integers(n)), PROB[ct])], False)
        hit = classes_of(plan_info(qsim, n, case, perm), n, gs, perm)
        got = [p for p in left if any(matches(p, k) for k in hit)]
        if got:
            out.append(case)
            left = [p for p in left if p not in got]
    return out


def search_relabeled(qsim, s, perm):
    """Cases for the labels `perm` a first run chose, which no fixed list can be steered for: the
    search for required_relabeled's role pair under perm."""
    return search_cases(qsim, s, required_relabeled(s)[:1], perm)


# ------------------------------------------------------------------------------ cases
_angle = fc._angle
# channel probabilities: one per type, all different, none with an exactly representable scale
PROB = {0: 0.07, 1: 0.23, 2: 0.31, 3: 0.11, 4: 0.17, 5: 0.29}


def cases(s, seed=4711):
    """List of (label, gates, channels, reference_y) for configuration `s`; gates = [(type, qubits,
    param)], channels = [(type, qubit or -1, p)].  Deterministic.  1 to 6 gates (after the anchor), one
    or two channels.  Prefix X gates claim register bits in program order, on the row side (high bits:
    first / last stages) and on the column side (low bits: middle stages) alike."""
    n = s["n"]
    h, rb, _ = shape(s)
    rng = np.random.default_rng(seed + 131 * n + 7 * h)
    ang = lambda: _angle(rng)
    g1 = lambda t, q: (t, [q], ang() if t >= RX else 0.0)
    pool = anchor_qubits(n) if s["anchor"] else list(range(n))
    out = []
    add = lambda label, gates, channels=(), ref_y=False: out.append((label, list(gates), list(channels), ref_y))
    orders = [pool, pool[::-1], pool[len(pool) // 2:] + pool[:len(pool) // 2]]
    width = max(1, rb)
    # -- gates alone: every 1-qubit type behind 0 .. rb-1 prefix gates, over three qubit orders
    for oi, order in enumerate(orders):
        for p in range(min(width, len(order) - 1)):
            pre = [g1(X, order[k]) for k in range(p)]
            tq = order[p]
            for t in ONE_Q:
                add(f"o{oi} p{p} {pc.NAMES[t]}[{tq}]", pre + [g1(t, tq)])
            for t in DIAG_Q:  # the X before claims the register bit
                add(f"o{oi} p{p} X {pc.NAMES[t]}[{tq}]", pre + [g1(X, tq), g1(t, tq)])
            if len(order) > width:  # the stage full of other bits: the diagonal's target a thread bit
                fill = [g1(X, q) for q in order[1:width + 1]]
                for t in DIAG_Q:
                    add(f"o{oi} thr {pc.NAMES[t]}[{order[0]}]", fill[:4] + [g1(t, order[0])])
    # -- two-qubit gates on every ordered pair of representatives, alone and behind a prefix
    reps = sorted({pool[0], pool[len(pool) // 2], pool[-1], pool[-2]})
    for a in reps:
        for b in reps:
            if a == b:
                continue
            for t in (CNOT, CZ) + ((SWAP,) if a < b else ()):
                add(f"{pc.NAMES[t]}[{a},{b}]", [(t, [a, b], 0.0)])
                others = [q for q in pool if q not in (a, b)][:width]
                add(f"fill {pc.NAMES[t]}[{a},{b}]", [g1(X, q) for q in others] + [(t, [a, b], 0.0)])
                add(f"H {pc.NAMES[t]}[{a},{b}]", [g1(H, a), (t, [a, b], 0.0)])
    # -- channels: each type after a gate that leaves the column bit a register bit (H, X: a 2x2 on
    #    it) or a thread bit (Z, T: diagonal), behind 0 .. rb-1 prefix gates on other qubits whose
    #    channels do not apply (the channel names its qubit)
    for oi, order in enumerate(orders):
        for p in range(min(width, len(order) - 1)):
            tq = order[p]
            for t in range(6):
                for gt in (H, X, Z, T, RY):
                    pre = [g1(X, order[k]) for k in range(p)]
                    add(f"o{oi} p{p} {pc.NAMES[gt]}[{tq}] ch{t}", pre + [g1(gt, tq)], [(t, tq, PROB[t])])
            # the stage opens with the channel's CX (the row bit its first register bit); the X
            # after it makes the column bit a register bit of the same stage
            for t in (0, 1, 3):
                pre = [g1(X, order[k]) for k in range(p)]
                add(f"o{oi} p{p} Z X[{tq}] ch{t}", pre + [g1(Z, tq), g1(X, tq)], [(t, tq, PROB[t])])
            # the column bit pushed out of the tile: wide prefixes
            for t in (0, 1, 3):
                wide = [g1(RY, q) for q in order if q != tq][:5]
                add(f"o{oi} wide p{p} ch{t}", wide + [g1(Z, tq)], [(t, tq, PROB[t])])
                add(f"o{oi} wide2 p{p} ch{t}", [g1(Z, tq)] + wide, [(t, tq, PROB[t])])
    # -- global channels on two-qubit gates, two-channel models, the reference's Y sign
    a, b = pool[0], pool[-1]
    for t in range(6):
        add(f"CNOT global ch{t}", [(CNOT, [a, b], 0.0)], [(t, -1, PROB[t])])
        add(f"SWAP CZ global ch{t},ch{(t + 1) % 6}", [(SWAP, [a, b], 0.0), (CZ, [b, a], 0.0)],
            [(t, -1, PROB[t]), ((t + 1) % 6, -1, PROB[(t + 1) % 6])])
    add("refY Y", [g1(Y, pool[0])], [], True)
    add("refY Y ch0", [g1(H, pool[-1]), g1(Y, pool[-1]), g1(Y, pool[0])], [(0, -1, PROB[0])], True)
    # -- mixed circuits over all types
    types = ONE_Q + [CNOT, CZ, SWAP]
    for k in range(16):
        gs = []
        for _ in range(int(rng.integers(3, 7))):
            t = int(rng.choice(types))
            qs = [int(q) for q in rng.choice(pool, size=1 if t <= RZ else 2, replace=False)]
            gs.append((t, qs, ang() if t in (RX, RY, RZ) else 0.0))
        t1, t2 = int(rng.integers(0, 6)), int(rng.integers(0, 6))
        chans = [(t1, -1 if k % 2 else int(rng.choice(pool)), PROB[t1])]
        if k % 3 == 0 and t2 != t1:
            chans.append((t2, int(rng.choice(pool)), PROB[t2]))
        add(f"mixed{k}", gs, chans, k % 8 == 7)
    for k, (gs, chans) in enumerate(STEERED.get(n, [])):
        if all(q in pool for _, qs, _ in gs for q in qs):
            add(f"steered{k}", gs, chans)
    if s["anchor"]:
        pre = [(Z, [q], 0.0) for q in anchor_qubits(n)]
        out = [(label, pre + gs, ch, ry) for label, gs, ch, ry in out]
    return out


# Circuits kept from search_cases (below: a seeded random search over the host planner, 1 to 6 gates
# and one channel) for the patterns of required() that the constructed cases above do not reach:
# mostly a channel or a controlled gate whose column bit lies outside the tile, which needs the pass
# full of other bits.  Per n: (gates, channels); channels as (type, qubit, PROB[type]).
STEERED = {
    5: [
        ([(CNOT, [0, 3], 0.0), (RX, [2], 1.012), (RY, [0], 0.867), (CZ, [1, 4], 0.0), (Z, [0], 0.0), (T, [3], 0.0)],
         [(0, 4, 0.07)]),
        ([(RX, [2], 1.152), (RX, [2], 0.923), (S, [3], 0.0)],
         [(1, 3, 0.23)]),
    ],
    6: [
        ([(SWAP, [3, 2], 0.0), (RY, [1], 0.458), (SDAG, [0], 0.0), (CZ, [5, 4], 0.0), (SWAP, [1, 4], 0.0), (CZ, [0, 3], 0.0)],
         [(0, 5, 0.07)]),  # (a gate op in a last stage at stage width 4)
        ([(CNOT, [4, 2], 0.0), (X, [3], 0.0), (Y, [1], 0.0), (CNOT, [1, 5], 0.0), (Z, [0], 0.0)],
         [(0, 4, 0.07)]),
        ([(CZ, [5, 1], 0.0), (Z, [0], 0.0), (TDAG, [4], 0.0), (TDAG, [3], 0.0), (TDAG, [2], 0.0), (SDAG, [1], 0.0)],
         [(0, 5, 0.07)]),
        ([(CZ, [4, 3], 0.0), (RZ, [3], 0.317), (S, [1], 0.0), (Z, [5], 0.0), (RX, [2], 1.042), (TDAG, [0], 0.0)],
         [(0, 4, 0.07)]),
    ],
    7: [
        ([(CNOT, [0, 2], 0.0), (CZ, [5, 1], 0.0), (RZ, [0], 0.265), (TDAG, [4], 0.0), (RX, [3], 1.005), (T, [6], 0.0)],
         [(3, 0, 0.11)]),
        ([(TDAG, [4], 0.0), (H, [3], 0.0), (CZ, [5, 1], 0.0), (T, [0], 0.0), (CZ, [6, 5], 0.0)],
         [(3, 6, 0.11)]),
        ([(CZ, [6, 1], 0.0), (Z, [0], 0.0), (TDAG, [5], 0.0), (TDAG, [4], 0.0), (TDAG, [3], 0.0), (SDAG, [1], 0.0)],
         [(0, 6, 0.07)]),
        ([(H, [6], 0.0), (CZ, [4, 0], 0.0), (CZ, [3, 2], 0.0), (TDAG, [3], 0.0), (SWAP, [3, 5], 0.0), (Y, [6], 0.0)],
         [(0, 4, 0.07)]),
        ([(SWAP, [1, 3], 0.0), (Z, [5], 0.0), (SWAP, [3, 2], 0.0), (Z, [2], 0.0)],
         [(3, 6, 0.11)]),
        ([(RY, [3], 0.681), (CNOT, [3, 4], 0.0), (SDAG, [4], 0.0)],
         [(3, 5, 0.11)]),
        ([(RZ, [1], 0.801), (RZ, [0], 0.529), (TDAG, [5], 0.0), (CNOT, [4, 6], 0.0), (H, [2], 0.0), (RY, [3], 1.33)],
         [(1, 6, 0.23)]),
    ],
    8: [
        ([(H, [6], 0.0), (X, [2], 0.0), (SWAP, [6, 0], 0.0), (CNOT, [3, 2], 0.0), (SWAP, [3, 4], 0.0), (SWAP, [1, 4], 0.0)],
         [(0, 2, 0.07)]),
        ([(CZ, [0, 5], 0.0), (Z, [6], 0.0), (Y, [6], 0.0)],
         [(3, 5, 0.11)]),
        ([(RY, [5], 0.517), (CZ, [7, 4], 0.0), (RZ, [1], 0.383), (T, [6], 0.0), (Y, [3], 0.0), (H, [3], 0.0)],
         [(1, 2, 0.23)]),
        ([(CZ, [6, 0], 0.0), (T, [7], 0.0), (T, [4], 0.0), (SDAG, [4], 0.0), (TDAG, [5], 0.0), (SDAG, [7], 0.0)],
         [(0, 6, 0.07)]),
        ([(SWAP, [5, 6], 0.0), (H, [6], 0.0), (RZ, [2], 1.122)],
         [(1, 2, 0.23)]),
        ([(RZ, [0], 0.497), (CZ, [7, 2], 0.0), (S, [1], 0.0), (RZ, [6], 0.631)],
         [(0, 7, 0.07)]),
        ([(S, [5], 0.0), (Y, [1], 0.0), (RX, [4], 0.89), (RZ, [3], 0.96), (X, [3], 0.0), (CZ, [6, 2], 0.0)],
         [(1, 6, 0.23)]),
        ([(X, [0], 0.0), (CZ, [5, 6], 0.0), (Z, [4], 0.0), (CZ, [7, 3], 0.0), (RY, [5], 0.418), (X, [2], 0.0)],
         [(3, 7, 0.11)]),
        ([(Z, [3], 0.0), (Y, [5], 0.0), (SDAG, [6], 0.0), (CZ, [6, 7], 0.0), (CNOT, [4, 5], 0.0)],
         [(0, 4, 0.07)]),
        ([(RZ, [6], 0.202), (X, [4], 0.0), (RX, [5], 1.177), (RZ, [5], 1.162), (SWAP, [6, 5], 0.0)],
         [(3, 7, 0.11)]),
        ([(X, [5], 0.0), (SWAP, [7, 6], 0.0), (CZ, [5, 6], 0.0), (T, [7], 0.0)],
         [(3, 3, 0.11)]),
        ([(RY, [5], 0.716), (Z, [6], 0.0), (CZ, [7, 3], 0.0), (SWAP, [7, 3], 0.0), (TDAG, [5], 0.0)],
         [(3, 6, 0.11)]),
        ([(SWAP, [7, 3], 0.0), (RY, [3], 0.216), (X, [3], 0.0), (RZ, [3], 1.362), (SWAP, [5, 7], 0.0), (RZ, [3], 0.564)],
         [(3, 6, 0.11)]),
        ([(RY, [3], 0.482), (SWAP, [4, 7], 0.0), (S, [7], 0.0), (H, [6], 0.0)],
         [(1, 6, 0.23)]),
        ([(H, [4], 0.0), (SWAP, [7, 3], 0.0), (SDAG, [3], 0.0), (Z, [4], 0.0), (RZ, [5], 0.817), (H, [6], 0.0)],
         [(3, 6, 0.11)]),
        ([(CNOT, [4, 7], 0.0), (SWAP, [4, 7], 0.0), (Z, [5], 0.0), (SDAG, [5], 0.0)],
         [(1, 6, 0.23)]),
        ([(Z, [4], 0.0), (Y, [3], 0.0), (CNOT, [3, 4], 0.0), (TDAG, [3], 0.0), (T, [6], 0.0), (Y, [4], 0.0)],
         [(3, 7, 0.11)]),
    ],
}


PREAMBLE_SEED = 99


def preamble(n):
    """The fixed first circuit of the relabeled configurations: wide enough that the first run's
    label search has something to gain, every channel type."""
    rng = np.random.default_rng(PREAMBLE_SEED + n)
    gs = []
    for layer in range(3):
        for q in range(n):
            t = int(rng.choice([H, RX, RY, T, X, RZ]))
            gs.append((t, [q], _angle(rng) if t >= RX else 0.0))
        perm = [int(q) for q in rng.permutation(n)]
        for a, b in zip(perm[::2], perm[1::2]):
            gs.append((int(rng.choice([CNOT, CZ])), [a, b], 0.0))
    return gs, [(0, -1, 0.02), (1, 1, 0.1), (3, n - 1, 0.05), (2, 0, 0.2)]


# ------------------------------------------------------------------------------ checks
def check(got, rho, want, may_change, info, jit=False, exact=None):
    """fused_cases.check on the flattened matrices."""
    return fc.check(np.asarray(got).reshape(-1), rho.reshape(-1), want.reshape(-1), may_change.reshape(-1),
                    info, jit=jit, exact=exact)


def err_of(got, want):
    return float(max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag))))


def pooled(s, per_circuit=16):
    """The gate lists of the cases of `s` that share a channel model, concatenated `per_circuit`
    gates at a time (one hipRTC compile per circuit; 16 gates of two ops each plus at most one
    channel of six ops per gate qubit keep a pass within kJitMaxOps = 192)."""
    groups = {}
    for _, gates, channels, ref_y in cases(dict(s, anchor=False)):
        if len(channels) <= 1:
            groups.setdefault((tuple(channels), ref_y), []).extend(gates)
    pre = [(Z, [q], 0.0) for q in anchor_qubits(s["n"])] if s["anchor"] else []
    out = []
    for (channels, ref_y), gates in groups.items():
        for i in range(0, len(gates), per_circuit):
            out.append((f"pooled{len(out)}", pre + gates[i:i + per_circuit], list(channels), ref_y))
    return out


def generated_circuits(qsim, s, perm=None, want=None):
    """The circuits configuration `s` runs through the generated kernels, as (index, case, info): a
    greedy cover of required(s) over the pooled circuits, then the cases on their own (pooling
    undoes their steering), among those whose passes are all staged and within kJitMaxOps (each
    circuit costs one hipRTC compile).  Deterministic."""
    n = s["n"]
    cand = []
    for k, case in enumerate(pooled(s) + cases(s)):
        info = plan_info(qsim, n, case, perm)
        if all(not p["single"] and p["rb"] > 0 and p["ops"] <= 192 for p in info["passes"]):
            cand.append((k, case, info))
    want = required(s) if want is None else want
    covers = []
    for _, case, info in cand:
        hit = classes_of(info, n, case[1], perm)
        covers.append({i for i, p in enumerate(want) if any(matches(p, key) for key in hit)})
    left, picked = set(range(len(want))), []
    while left:
        best = max(range(len(cand)), key=lambda c: (len(covers[c] & left), -c))
        if not covers[best] & left:
            break  # (a required class no case reaches: the caller's coverage assertion reports it)
        picked.append(best)
        left -= covers[best]
    return [cand[c] for c in sorted(picked)]


def run_matrix(qsim, s, modes=None, case_list=None, stop_at=6):
    """Every case of `s`: dense rho -> state.fromHost -> DensityMatrixSimulator.run ->
    getDensityMatrix against the reference (computed once per case), in every run mode of `modes`
    (default: fused, then per-gate).  Returns (cases run, worst error, failures, classes)."""
    n = s["n"]
    modes = (qsim.RunMode.Fused, qsim.RunMode.PerGate) if modes is None else modes
    case_list = cases(s) if case_list is None else case_list
    sims = [qsim.DensityMatrixSimulator(n, mode=m) for m in modes]
    ran, worst, failures, hit = 0, 0.0, [], set()
    for k, case in enumerate(case_list):
        if len(failures) >= stop_at:
            break
        label, gates, channels, ref_y = case
        info = plan_info(qsim, n, case)
        hit |= classes_of(info, n, gates)
        rho = dense_rho(n, 1000 * n + k)
        want, may = reference(n, rho, gates, channels, ref_y)
        c, nm = circuit_of(qsim, n, gates), noise_of(qsim, channels)
        ran += 1
        for sim, mode in zip(sims, modes):
            sim.setNoiseModel(nm)
            sim.setReferenceCompatible(ref_y)
            sim.density.state.fromHost(rho.reshape(-1))
            sim.run(c)
            try:
                worst = max(worst, check(sim.getDensityMatrix(), rho, want, may, info))
            except AssertionError as e:
                failures.append(f"{s['name']} {label} {mode.name}: {e}")
    return ran, worst, failures, hit


def run_channels(qsim, n):
    """applyChannel of every type on every qubit from the dense matrix (the per-gate kernels on the
    lowered sequence).  Returns (cases, worst error, failures)."""
    sim = qsim.DensityMatrixSimulator(n)
    rho = dense_rho(n, 31 + n)
    ran, worst, failures = 0, 0.0, []
    for t in range(6):
        for q in range(n):
            want, may = channel(n, rho, t, q, PROB[t])
            sim.density.state.fromHost(rho.reshape(-1))
            sim.applyChannel(qsim.NoiseType(t), q, PROB[t])
            got = sim.getDensityMatrix()
            ran += 1
            try:
                keep = ~may
                assert np.array_equal(got[keep].view(np.uint64), rho[keep].view(np.uint64)), \
                    "elements outside the channel's mask changed"
                err = err_of(got, want)
                worst = max(worst, err)
                assert err <= TOL, f"max component error {err:.3e} > {TOL:g}"
            except AssertionError as e:
                failures.append(f"n={n} {CH_NAMES[t]}[{q}]: {e}")
    return ran, worst, failures


def run_generated(qsim, s):
    """generated_circuits(s) through the generated kernels (the caller set set_jit(2, 0)); every
    staged pass must have run as one.  Returns (circuits, worst error, failures, classes)."""
    n = s["n"]
    sim = qsim.DensityMatrixSimulator(n)
    ran, worst, failures, hit = 0, 0.0, [], set()
    for k, case, info in generated_circuits(qsim, s):
        label, gates, channels, ref_y = case
        rho = dense_rho(n, 5000 * n + k)
        want, may = reference(n, rho, gates, channels, ref_y)
        sim.setNoiseModel(noise_of(qsim, channels))
        sim.setReferenceCompatible(ref_y)
        sim.density.state.fromHost(rho.reshape(-1))
        sim.run(circuit_of(qsim, n, gates))
        passes, jp = sim.density.state.lastRunInfo()
        ran += 1
        try:
            assert jp == passes == len(info["passes"]) >= 1, f"{jp} of {passes} passes ran as generated kernels"
            worst = max(worst, check(sim.getDensityMatrix(), rho, want, may, info, jit=True))
        except AssertionError as e:
            failures.append(f"{s['name']} {label}: {e}")
            break
        hit |= classes_of(info, n, gates)
    return ran, worst, failures, hit


def run_relabeled(qsim, s, jit=False, stop_at=4):
    """The relabeled configurations: from a reset rho a first fused run of preamble(n), which takes
    relabeled index bits; the case runs second with no reader in between; perm() is read before
    getDensityMatrix restores the identity layout; the result is compared with the reference of
    preamble plus case at 1e-12 and the classes come from the plan under that perm.  With jit only
    the greedy cover under the labels runs.  Returns (cases, worst, failures, classes)."""
    n = s["n"]
    pre_g, pre_ch = preamble(n)
    rho0 = np.zeros((1 << n, 1 << n), np.complex128)
    rho0[0, 0] = 1.0
    base, _ = reference(n, rho0, pre_g, pre_ch)
    sim = qsim.DensityMatrixSimulator(n)
    pre_c = circuit_of(qsim, n, pre_g)

    def first_run():
        sim.reset()
        sim.setNoiseModel(noise_of(qsim, pre_ch))
        sim.setReferenceCompatible(False)
        sim.run(pre_c)
        return sim.density.state.perm()

    perm = first_run()
    assert perm != list(range(2 * n)), "the first run did not relabel"
    todo = ([(k, case) for k, case, _ in generated_circuits(qsim, s, perm, required_relabeled(s) + required(s))]
            if jit else list(enumerate(cases(s))))
    todo += [(10000 + k, case) for k, case in enumerate(search_relabeled(qsim, s, perm))]
    ran, worst, failures, hit = 0, 0.0, [], set()
    for k, case in todo:
        if len(failures) >= stop_at:
            break
        label, gates, channels, ref_y = case
        assert first_run() == perm  # (memoised per circuit structure)
        info = plan_info(qsim, n, case, perm)
        want, _ = reference(n, base, gates, channels, ref_y)
        sim.setNoiseModel(noise_of(qsim, channels))
        sim.setReferenceCompatible(ref_y)
        sim.run(circuit_of(qsim, n, gates))
        ran += 1
        try:
            assert sim.density.state.perm() == perm, "the second run changed the labels"
            if jit:
                passes, jp = sim.density.state.lastRunInfo()
                assert jp == passes == len(info["passes"]) >= 1, (
                    f"{jp} of {passes} passes ran as generated kernels, {len(info['passes'])} planned")
            err = err_of(sim.getDensityMatrix(), want)
            worst = max(worst, err)
            assert err <= TOL, f"max component error {err:.3e} > {TOL:g}"
        except AssertionError as e:
            failures.append(f"{s['name']} {label}: {e}")
        hit |= classes_of(info, n, gates, perm)
    return ran, worst, failures, hit
