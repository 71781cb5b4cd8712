"""Operand-class cases, class keys and checks for the fused pass kernels (csrc/hip/fused.hip
k_fused_tile / k_fused_staged and the generated kernels of jit.hip).

Helper module (no tests here), shared by tests/test_fused_matrix_cpu.py,
tests/test_fused_matrix_gpu.py and the child script tests/fused_child.py.

  * `reference`: the circuit applied gate by gate with pergate_cases.dense_apply (plain numpy,
    independent of the engine and of oracle/); returns the state and the OR of the gates'
    may-change masks.
  * `class_of`: the class key of one record of plan.plan_stage_info, i.e. the branch of the pass
    kernels the op takes: (family, stage position, arm, target role, control roles, d0_one, r0).
  * `cases`: short circuits (1 to 6 gates) built so that the planner puts operands into the roles
    wanted; prefix gates on other qubits, claiming register bits in program order, steer it.
  * `required`: the class patterns a configuration must hit, written from the kernels' branches.
  * `generated_circuits`: the few circuits per configuration that go through the generated
    kernels, pooled cases plus the steered cases needed to cover `required`.
  * `check`: bit-identity outside the may-change mask, tolerance 0 for circuits of exact ops, the
    project's 1e-12 per component otherwise.

Out of scope here: the Pauli-frame arms (FR = true, batched noisy runs) and sub-space launches
(fix_mask, the sharded engine), each with oracle tests of its own, and the density-matrix passes,
which have this module's counterpart in tests/dm_pass_cases.py.
"""
import math

import numpy as np

import pergate_cases as pc
from pergate_cases import (X, Y, Z, H, S, T, SDAG, TDAG, RX, RY, RZ, CNOT, CZ, CRY, CRZ, SWAP,  # noqa: F401
                           TOFFOLI)

TOL = pc.TOL  # the project's bar per real and imaginary component (test_parity_gpu.TOL)
K_M1, K_DIAG, K_SWAP = 0, 1, 2
S_GEN, S_X, S_Y, S_H, S_NEG, S_I, S_MI, S_T, S_TDG = range(9)
ANY = None  # wildcard of a required pattern

# Ops whose arm does no rounding arithmetic, as (kind, sub).
#   k_fused_tile and the per-gate fallback (device_ops.hpp m1_pair / diag1): S_X swaps, S_Y swaps
#   components and negates, S_NEG negates, S_I / S_MI swap components and negate, K_SWAP moves.
#   k_fused_staged: A_SWAP (S_X, the SWAP lowering) is selects only; S_Y runs through A_GEN as
#   cmul by 0 and -+i and the sum with an exact zero (a product by 0 or 1 is exact, also when it is
#   contracted into an FMA); stage_diag's NEG arm negates; S_I / S_MI are cmul by +-i in the phase
#   arm; the store multiplies by scale == 1.0 when the pass holds no unnormalised H.
#   Generated kernels (jit.hip Gen::op_body, Gen::diag1): S_X is a rename or a select, S_Y, S_NEG,
#   S_I, S_MI are written as component moves and negations, no product feeds a sum in them, so
#   contraction has nothing to fuse; the store scale is omitted or 1.0.
# A circuit is compared at tolerance 0 when every op is in the set and no pass has hu_count > 0.
EXACT_OPS = frozenset({(K_M1, S_X), (K_M1, S_Y), (K_DIAG, S_NEG), (K_DIAG, S_I), (K_DIAG, S_MI),
                       (K_SWAP, S_GEN)})
EXACT_OPS_JIT = EXACT_OPS


# ------------------------------------------------------------------------------ settings
def settings(name, n, h=None, rb7=None, ctrl_out=1, env=None, anchor=True):
    """One configuration: the state size, a forced tile height (None: the size rule), the stage
    width of 13-qubit tiles, tile-constant controls, and per-process knobs (children only).
    anchor (h = 7 only): every case starts with Z on qubits 4..12.  plan_fused (QSIM_TILE_MIX)
    demotes a pass of a 13-qubit plan to a 12-qubit tile when its gates fit one at some run width
    r0 in 4..6, which every short circuit does; gates on nine qubits from 4 up fit none, so the
    pass keeps h = 7.  Diagonal ops claim no register bit, so the anchors leave the stages of the
    gates under test as they are.  anchor = False is the demotion itself."""
    return {"name": name, "n": n, "h": h, "rb7": rb7, "ctrl_out": ctrl_out, "env": dict(env or {}),
            "anchor": anchor and h == 7}


def apply_settings(plan, s):
    plan.set_tile_height(-1 if s["h"] is None else s["h"])
    plan.set_tile_rb7(-1 if s["rb7"] is None else s["rb7"])
    plan.set_tile_ctrl_out(s["ctrl_out"])


def restore_settings(plan):
    plan.set_tile_rb7(-1)
    plan.restore_defaults()


def shape(s):
    """(h, rb, r0) of the passes the size rules of fused.hip give this configuration (rb = 0:
    unstaged tiles); tile_rb_for: 3 for 12-qubit tiles from 12 to 20 qubits unless QSIM_TILE_RB."""
    n, env = s["n"], s["env"]
    h = min(6 if s["h"] is None else s["h"], n - 6)
    if h == 7 and not s["anchor"]:
        return 6, 4, int(env.get("QSIM_TILE_R0", 6))  # demoted: stage_rb(6), not the small-state width
    if h < 4:
        return h, 0, 6
    if h == 7:
        rb = s["rb7"] or 4
    elif h == 6:
        rb = int(env.get("QSIM_TILE_RB", 3 if 12 <= n <= 20 else 4))
    else:
        rb = h - 2
    return h, rb, int(env.get("QSIM_TILE_R0", 6))


# The in-process configurations of tests/test_fused_matrix_gpu.py.
NATURAL = [settings(f"n{n}", n) for n in (6, 7, 8, 9, 10, 11, 12, 13, 14)]
FORCED = ([settings(f"h{h}_n{h + 8}", h + 8, h=h) for h in range(6)] +
          [settings("h7rb4_n14", 14, h=7, rb7=4), settings("h7rb3_n14", 14, h=7, rb7=3),
           settings("h7rb4_n15", 15, h=7, rb7=4), settings("h7rb3_n15", 15, h=7, rb7=3),
           settings("h7mix_n14", 14, h=7, anchor=False)])
CTRL_OUT_OFF = [settings("n13_co0", 13, ctrl_out=0), settings("h4_n12_co0", 12, h=4, ctrl_out=0)]
IN_PROCESS = NATURAL + FORCED + CTRL_OUT_OFF
# Generated kernels (set_jit(2, 0)): every configuration with staged tiles (jit.hip specialises
# passes of h >= 4 only).
GENERATED = [c for c in IN_PROCESS if min(6 if c["h"] is None else c["h"], c["n"] - 6) >= 4]
# Knobs read once per process: each variant runs in a child (tests/fused_child.py).  "jit": the
# child runs generated_circuits through the generated kernels instead of the case matrix.
KNOBS = ("QSIM_TILE_RB", "QSIM_TILE_R0", "QSIM_FUSED_NT", "QSIM_JIT_NT", "QSIM_JIT_PIPE", "QSIM_JIT_XCD",
         "QSIM_PLANNER", "QSIM_STAGE_SEARCH", "QSIM_TILE_HMAX", "QSIM_TILE_RB7", "QSIM_TILE_CTRL_OUT",
         "QSIM_TILE_MIX", "QSIM_STAGE_BEAM", "QSIM_JIT", "QSIM_JIT_MIN_QUBITS")
CHILDREN = [
    # k_fused_staged<6, ., false, 4>, the instantiation of every state from 21 qubits
    [settings("rb4_n13", 13, env={"QSIM_TILE_RB": 4}), settings("rb4_n14", 14, env={"QSIM_TILE_RB": 4})],
    [settings("rb4_nt0_n13", 13, env={"QSIM_TILE_RB": 4, "QSIM_FUSED_NT": 0}),
     settings("rb4_nt0_n14", 14, env={"QSIM_TILE_RB": 4, "QSIM_FUSED_NT": 0})],
    [settings("rb2_n13", 13, env={"QSIM_TILE_RB": 2})],
    [settings("r0_4_n13", 13, env={"QSIM_TILE_R0": 4})],  # r0 < 6: run_mask, four runs per wave load
    [settings("r0_5_n13", 13, env={"QSIM_TILE_R0": 5})],
    [settings("firstfit_n13", 13, env={"QSIM_STAGE_SEARCH": 0, "QSIM_PLANNER": 0})],
    [dict(settings("jit_nt0_n13", 13, env={"QSIM_JIT_NT": 0, "QSIM_JIT_XCD": 0, "QSIM_JIT_PIPE": 0}), jit=True),
     dict(settings("jit_nt0_h7", 14, h=7, rb7=4, env={"QSIM_JIT_NT": 0, "QSIM_JIT_XCD": 0, "QSIM_JIT_PIPE": 0}),
          jit=True)],
    # QSIM_JIT_PIPE (jit.hip jit_pass_pipelined): 0 never, 1 13-qubit tiles only, 2 every multi-stage pass
    [dict(settings("jit_pipe2_n13", 13, env={"QSIM_JIT_PIPE": 2}), jit=True),
     dict(settings("jit_pipe2_h7", 14, h=7, rb7=4, env={"QSIM_JIT_PIPE": 2}), jit=True)],
]


# ------------------------------------------------------------------------------ reference
def circuit_of(qsim, n, gates):
    c = qsim.Circuit(n)
    for t, qs, p in gates:
        c.append(qsim.GateOp(t, list(qs), p))
    return c


def reference(n, psi, gates):
    """(state, may_change) of the gate list on psi by pergate_cases.dense_apply, gate by gate."""
    out = np.asarray(psi, np.complex128)
    may = np.zeros(1 << n, bool)
    for t, qs, p in gates:
        out, m = pc.dense_apply(n, out, t, qs, p)
        may |= m
    return out, may


def dense_state(n, seed):
    """Dense normalised complex Gaussian vector (no zero components, so no signed zeros arise)."""
    return pc.random_state(n, seed)


# ------------------------------------------------------------------------------ class keys
def class_of(rec, ps):
    """Class key of op record `rec` in pass record `ps` (plan.plan_stage_info):
    (family, position, arm, target role, control roles, d0_one, r0).
      family    "single" (per-gate fallback), "tile<h>" (k_fused_tile<h>) or ("staged", h, rb)
      position  first / middle / last / only (stage_begin loads from HBM, stage_end - 1 stores)
      arm       staged 2x2: swap / hu / gen (stage_m1_arm); staged diagonal: neg / phase
                (stage_op); unstaged: m1 / diag / swap (the three branches of k_fused_tile)
      target    staged 2x2: p<p0>; staged diagonal: p<p0>, or thr_lo / thr_hi for a thread bit
                below / from tile bit 4 (the LDS swizzle XORs bits 0-3); unstaged: lane (< 6) or
                high (spread over hpos); SWAP: the pair of both
      controls  sorted tuple of reg / thr / out (unstaged: tile)
    """
    if ps["single"]:
        return ("single", "only", "gate", "", (), rec["d0_one"], 6)
    ncm = bin(rec["cmask"]).count("1")
    if ps["rb"] == 0:
        role = lambda b: "lane" if b < 6 else "high"
        arm = {K_M1: "m1", K_DIAG: "diag", K_SWAP: "swap"}[rec["kind"]]
        tgt = role(rec["b0"]) + ("+" + role(rec["b1"]) if rec["kind"] == K_SWAP else "")
        return (f"tile{ps['h']}", "only", arm, tgt, ("tile",) * ncm, rec["d0_one"], ps["r0"])
    ctl = (("reg",) * bin(rec["cm_reg"]).count("1") + ("thr",) * bin(rec["cm_thr"]).count("1") +
           ("out",) * bin(rec["cm_out"]).count("1"))
    if rec["kind"] == K_DIAG:
        arm = "neg" if rec["sub"] == S_NEG else "phase"
        tgt = f"p{rec['p0']}" if rec["p0"] >= 0 else ("thr_lo" if rec["b0"] < 4 else "thr_hi")
    else:
        arm = {S_X: "swap", S_H: "hu"}.get(rec["sub"], "gen")
        tgt = f"p{rec['p0']}"
    return (("staged", ps["h"], ps["rb"]), rec["pos"], arm, tgt, tuple(sorted(ctl)), rec["d0_one"], ps["r0"])


def classes_of(info):
    return {class_of(r, info["passes"][r["pass"]]) for r in info["ops"]}


def matches(pattern, key):
    return all(p is ANY or p == k for p, k in zip(pattern, key))


def missing(required_patterns, hit):
    return [p for p in required_patterns if not any(matches(p, k) for k in hit)]


def required(s):
    """The class patterns configuration `s` must hit (ANY = any value), from the kernels' branches.

    Unstaged (k_fused_tile<h>, fused.hip): the K_M1 sweep with and without controls and with the
    target on a lane bit and, for h > 0, on a high bit (ins0 above bit 5, spread over hpos); the
    two K_DIAG loops (d0_one / two-sided); K_SWAP low/low and, for h > 0, low/high.
    Tile-constant controls do not exist there (append_tile_pass refuses cm_out below h = 4 and
    choose_passes only lets controls out of tiles of at least 10 bits: `co = tile_ctrl_out() &&
    nfree + r0 >= 10`), so a control outside the tile makes the gate a per-gate step: "single".

    Staged (k_fused_staged<h, ., false, rb>): stage_op dispatches on p0 < rb, stage_m1_arm on
    swap / hu / gen and on PRED; the control test has three parts (cm_reg scalar, cm_thr per lane,
    cm_out on the load base), alone and paired (Toffoli); stage_diag has the NEG and the phase arm,
    the target on each register bit or on a thread bit, one- and two-sided; every stage position
    loads and stores differently.  Left out as unreachable by construction:
      * a controlled A_HU: no controlled H in the gate set, and plan_stages relabels any to S_GEN
        (`if (t.cmask == 0 && t.cm_out == 0 && ...) ++p.hu_count; else t.sub = S_GEN`);
      * cm_out where no qubit lies outside the tile (n == 6 + h), or with set_tile_ctrl_out(0);
      * two reg controls at rb = 2 (the target takes one of the two register bits);
      * a 2x2 op in the first or last stage with a register bit below tile bit 6 (both stages
        only take high tile bits: `take(from, high_bits)` / `(seq.back().first & ~st_high) == 0`).
    """
    n = s["n"]
    h, rb, r0 = shape(s)
    out = []
    if rb == 0:
        fam = f"tile{h}"
        out += [(fam, "only", "m1", "lane", (), ANY, 6), (fam, "only", "m1", "lane", ("tile",), ANY, 6),
                (fam, "only", "m1", "lane", ("tile", "tile"), ANY, 6),
                (fam, "only", "diag", "lane", (), 1, 6), (fam, "only", "diag", "lane", (), 0, 6),
                (fam, "only", "diag", "lane", ("tile",), 1, 6), (fam, "only", "diag", "lane", ("tile",), 0, 6),
                (fam, "only", "swap", "lane+lane", (), ANY, 6)]
        if h > 0:
            out += [(fam, "only", "m1", "high", (), ANY, 6), (fam, "only", "m1", "high", ("tile",), ANY, 6),
                    (fam, "only", "diag", "high", (), 1, 6), (fam, "only", "diag", "high", (), 0, 6),
                    (fam, "only", "swap", "lane+high", (), ANY, 6)]
        if n > 6 + h and h < 3:  # more operands from qubit 6 up than free slots: the per-gate fallback
            out.append(("single", ANY, ANY, ANY, ANY, ANY, ANY))
        return out
    fam = ("staged", h, rb)
    has_out = n > 6 + h and s["ctrl_out"] == 1
    for p in range(rb):
        tgt = f"p{p}"
        for arm in ("swap", "hu", "gen"):
            out.append((fam, ANY, arm, tgt, (), ANY, r0))                 # PRED = false
        for arm in ("swap", "gen"):
            out.append((fam, ANY, arm, tgt, ("thr",), ANY, r0))           # PRED = true
        out += [(fam, ANY, "neg", tgt, ANY, 1, r0), (fam, ANY, "phase", tgt, ANY, 1, r0),
                (fam, ANY, "phase", tgt, ANY, 0, r0)]
    for tgt in ("thr_lo", "thr_hi"):
        out += [(fam, ANY, "neg", tgt, ANY, 1, r0), (fam, ANY, "phase", tgt, ANY, 1, r0),
                (fam, ANY, "phase", tgt, ANY, 0, r0)]
    roles = ["reg", "thr"] + (["out"] if has_out else [])
    for c in roles:  # one control of each role on every arm that takes controls
        for arm in ("swap", "gen", "neg", "phase"):
            out.append((fam, ANY, arm, ANY, (c,), ANY, r0))
        out.append((fam, ANY, "phase", ANY, (c,), 0, r0))  # CRZ: two-sided under a control
    for i, a in enumerate(roles):  # Toffoli: every pairing
        for b in roles[i:]:
            if (a, b) == ("reg", "reg") and rb < 3:
                continue
            if (a, b) == ("out", "out") and n < 6 + h + 2:  # (needs two qubits outside the tile)
                continue
            out.append((fam, ANY, "swap", ANY, tuple(sorted((a, b))), ANY, r0))
    for pos in ("first", "middle", "last", "only"):
        for arm in ("swap", "gen", "hu"):
            out.append((fam, pos, arm, ANY, ANY, ANY, r0))
        out.append((fam, pos, "phase", ANY, ANY, ANY, r0))
    # the middle stages reach tile bits 0-3 and 4-5 as register bits; diagonals on thread bits in
    # a middle stage read jb after the LDS round trip
    out += [(fam, "middle", "neg", "thr_lo", ANY, ANY, r0), (fam, "middle", "phase", "thr_hi", ANY, ANY, r0)]
    return out


# ------------------------------------------------------------------------------ cases
def _angle(rng):
    return float(int(rng.integers(0, 4)) * (math.pi / 2) + rng.uniform(0.1, math.pi / 2 - 0.1))


ANCHOR = [(Z, [q], 0.0) for q in range(4, 13)]


def cases(s, seed=2025, anchor=True):
    """List of (label, gates, expect_single) for configuration `s`; gates = [(type, qubits, param)].
    Deterministic.  Qubits 0-5 are the lanes of every tile; hi[] are the qubits from 6 up that the
    planner's padding puts into a tile of 6 + h bits when no gate asks for others (the lowest
    ones), out[] the topmost qubits, outside such a tile when n > 6 + h."""
    n = s["n"]
    h, rb, _ = shape(s)
    tb = 6 + h
    rng = np.random.default_rng(seed + 131 * n + 7 * h)
    ang = lambda: _angle(rng)
    g1 = lambda t, q: (t, [q], ang() if t >= RX else 0.0)
    g2 = lambda t, a, b: (t, [a, b], ang() if t in (CRY, CRZ) else 0.0)
    tof = lambda a, b, t: (TOFFOLI, [a, b, t], 0.0)
    hi = list(range(6, min(tb, n)))                 # high tile qubits by default
    outside = [q for q in (n - 1, n - 2) if q >= tb]  # outside the default tile
    out = []
    staged = rb > 0
    # tile-constant controls exist for staged tiles only; elsewhere an outside control is a
    # per-gate step
    co = staged and s["ctrl_out"] == 1

    def single(gates):
        """A gate becomes a per-gate step when the qubits from 6 up that its tile must hold (its
        targets; without tile-constant controls its controls too) outnumber the h free slots."""
        for t, qs, _ in gates:
            need = qs if (t == SWAP or not co) else qs[-1:]
            if len({q for q in need if q >= 6}) > h:
                return True
        return False

    add = lambda label, gates: out.append((label, list(gates), single(gates)))

    # -- one gate: every one-qubit type on a lane bit below 4, a lane bit from 4, the first and
    #    the last high tile qubit, and the top qubit (hpos then skips positions)
    ones = [0, 3, 5] + hi[:1] + hi[-1:] + [n - 1]
    ones = sorted({q for q in ones if q < n})
    for q in ones:
        for t in range(X, RZ + 1):
            add(f"{pc.NAMES[t]}[{q}]", [g1(t, q)])
    # -- one controlled gate on every ordered pair of representatives
    reps = sorted({q for q in [0, 5] + hi[:1] + hi[-1:] + [n - 1] + outside if q < n})
    for a in reps:
        for b in reps:
            if a == b:
                continue
            for t in (CNOT, CZ, CRY, CRZ):
                add(f"{pc.NAMES[t]}[{a},{b}]", [g2(t, a, b)])
            if a < b:
                add(f"SWAP[{a},{b}]", [(SWAP, [a, b], 0.0)])
    # -- Toffoli: controls low (thread bits of a first stage), high (register bits by padding),
    #    outside (tile-constant), in every pairing, target high and low
    if hi:
        t_hi, t_lo = hi[-1], 2
        pools = {"lo": [0, 4], "hi": hi[:2] if len(hi) >= 3 else hi[:1], "out": outside}
        kinds = ["lo", "hi", "out"]
        for i, ka in enumerate(kinds):
            for kb in kinds[i:]:
                pa, pb = pools[ka], pools[kb]
                if not pa or not pb:
                    continue
                a = pa[0]
                b = pb[0] if pb[0] != a else (pb[1] if len(pb) > 1 else None)
                if b is None:
                    continue
                for t in (t_hi, t_lo):
                    if t in (a, b):
                        continue
                    add(f"Toffoli[{a},{b},{t}]", [tof(a, b, t)])
                    add(f"Toffoli[{b},{a},{t}]", [tof(b, a, t)])
    else:
        add("Toffoli[0,4,2]", [tof(0, 4, 2)])
        add("Toffoli[5,1,3]", [tof(5, 1, 3)])
    # -- SWAP inside the tile next to gates controlled from outside it
    if outside:
        c = outside[0]
        if len(hi) >= 2:
            add(f"ctx SWAP[{hi[0]},{hi[-1]}]", [g2(CNOT, c, hi[0]), (SWAP, [hi[0], hi[-1]], 0.0), g2(CZ, c, hi[-1])])
        add("ctx SWAP[1,4]", [g2(CRY, c, 1), (SWAP, [1, 4], 0.0), g2(CRZ, c, 4)])
    if staged:
        _staged_cases(s, g1, g2, tof, hi, outside, add)
    # -- a few mixed circuits of 3 to 6 gates over all types
    for k in range(12):
        gs = []
        for _ in range(int(rng.integers(3, 7))):
            t = int(rng.integers(0, 17))
            qs = [int(q) for q in rng.choice(min(n, max(tb, 7)), size=1 if t <= RZ else 2 if t <= SWAP else 3,
                                             replace=False)]
            gs.append((t, qs, ang() if t in (RX, RY, RZ, CRY, CRZ) else 0.0))
        out.append((f"mixed{k}", gs, None))  # (None: either way; the planner decides)
    if s["anchor"] and anchor:
        out = [(label, ANCHOR + gs, single) for label, gs, single in out]
    return out


def _staged_cases(s, g1, g2, tof, hi, outside, add):
    """Steered cases for the register stages.  The first stage takes 2x2 ops on high tile bits only
    and claims register bits in program order, then pads with its ops' control bits, then with the
    highest bits; an op whose bits a deferred op touches is deferred too."""
    h, rb, _ = shape(s)
    one_q = [X, H, RY, Y, RX]            # swap, hu and gen arms
    diag_q = [Z, S, T, TDAG, SDAG, RZ]   # neg, one-sided and two-sided phase
    # target on register bit p of the first stage: X on the p lower high qubits first
    for p in range(min(rb, len(hi))):
        pre = [g1(X, hi[k]) for k in range(p)]
        tq = hi[p]
        for t in one_q:
            add(f"p{p} {pc.NAMES[t]}", pre + [g1(t, tq)])
        for t in diag_q:  # (a diagonal claims no register bit: the X before it does)
            add(f"p{p} {pc.NAMES[t]}", pre + [g1(X, tq), g1(t, tq)])
        for t in (X, H, RY, RZ):  # the same stage, now followed by a middle one
            add(f"p{p} {pc.NAMES[t]} then low", pre + [g1(t, tq), g1(X, 0)])
        for c in (0, 5):  # a thread-bit control: low qubits are never first-stage register bits
            for t in (CNOT, CRY, CZ, CRZ):
                add(f"p{p} {pc.NAMES[t]} c{c}", pre + [g2(t, c, tq)])
    # the same in a middle stage: low targets, register bits claimed in program order
    for p in range(rb):
        lows = [0, 1, 3, 4, 5]
        pre = [g1(X, lows[k]) for k in range(p)]
        tq = lows[p]
        for t in one_q:
            add(f"mid p{p} {pc.NAMES[t]}", pre + [g1(t, tq)])
        for t in diag_q:
            add(f"mid p{p} {pc.NAMES[t]}", pre + [g1(X, tq), g1(t, tq)])
        free = [q for q in (2, 5) if q not in lows[:p + 1]][0]
        fill = [g1(X, q) for q in lows[p + 1:rb]]  # fill the stage: the control stays a thread bit
        for t in (CNOT, CRY, CZ, CRZ):
            add(f"mid p{p} {pc.NAMES[t]} thr", pre + fill + [g2(t, free, tq)])
            add(f"mid p{p} {pc.NAMES[t]} reg", pre + [g2(t, free, tq)])
            if hi:
                add(f"mid p{p} {pc.NAMES[t]} hi", pre + [g2(t, hi[-1], tq)])
            if outside:
                add(f"mid p{p} {pc.NAMES[t]} out", pre + [g2(t, outside[0], tq)])
    # diagonal on a thread bit of a middle stage: the stage's register bits are full
    fill = [g1(X, q) for q in (1, 2, 4, 5)[:rb]]
    for t, q in ((Z, 0), (Z, 3), (T, 0), (RZ, 3), (S, hi[0]), (RZ, hi[-1]), (CZ, hi[0])):
        gate = g1(t, q) if t != CZ else g2(CZ, q, 0)
        # (blocked behind the X on qubit 1 by a CZ that shares it, so it cannot run first)
        add(f"mid thr {pc.NAMES[t]}[{q}]", fill + [g2(CZ, 1, q) if q != 1 else g1(Z, 1), gate])
    # ops in the last stage: a chain H(0), CNOT(0 -> 1), ... in which every gate needs the one
    # before and a register bit of its own fills a middle stage's rb bits whatever bits the stage
    # search tries; the next link, with a high target, opens a stage of high bits only, which then
    # stores straight to HBM
    low = [g1(H, 0)] + [g2(CNOT, k, k + 1) for k in range(rb - 1)]
    tq = hi[-1]
    for t in (CNOT, CRY, CZ, CRZ):
        add(f"last {pc.NAMES[t]}", low + [g2(t, rb - 1, tq)])
    for t in (X, H, RY, Z, T, RZ):
        add(f"last {pc.NAMES[t]}", low + [g2(CNOT, rb - 1, tq), g1(t, tq)])
    if len(hi) >= 3:
        add("last Toffoli", low + [tof(rb - 1, hi[0], tq)])
    if outside:
        add("last CNOT out", low + [g2(CNOT, rb - 1, tq), g2(CRY, outside[0], tq)])


def many_h_circuit(n=12, count=600, seed=11):
    """`count` H cycling over all n qubits, interleaved with T and Rz on the qubit just used so that
    no two H are adjacent on a qubit: one 12-qubit pass holds more than kMaxUnnormH = 512 of them."""
    rng = np.random.default_rng(seed)
    gs = []
    for k in range(count):
        q = k % n
        gs.append((H, [q], 0.0))
        gs.append((T, [q], 0.0) if k % 2 else (RZ, [q], _angle(rng)))
    return gs


def pooled(s, per_circuit=56):
    """The gate lists of the cases of `s` concatenated into few circuits (generated kernels: one
    hipRTC compile per circuit; the anchor once per circuit).  56 gates keep a pass within the 192
    ops a generated pass may hold (jit.hip kJitMaxOps; a SWAP is three ops), beyond which a pass
    stays on the interpreter.  Cases that expect, or may get, a per-gate step are left out."""
    gates = [g for _, gs, single in cases(s, anchor=False) if single is False for g in gs]
    pre = ANCHOR if s["anchor"] else []
    return [pre + gates[i:i + per_circuit] for i in range(0, len(gates), per_circuit)]


# ------------------------------------------------------------------------------ checks
def is_exact(info, jit=False):
    exact = EXACT_OPS_JIT if jit else EXACT_OPS
    return (all((r["kind"], r["sub"]) in exact for r in info["ops"]) and
            all(p["hu_count"] == 0 for p in info["passes"]))


def check(got, psi, want, may_change, info, jit=False, exact=None):
    """Asserts, in this order: amplitudes outside may_change are bit-identical to the input whenever
    no pass has an unnormalised H (its store scale is then exactly 1); a circuit of exact ops
    equals the reference at tolerance 0; otherwise max(|dRe|, |dIm|) <= 1e-12.  Returns the largest
    component error."""
    got = np.ascontiguousarray(got, np.complex128)
    assert got.shape == psi.shape == want.shape == may_change.shape
    if all(p["hu_count"] == 0 for p in info["passes"]):
        keep = ~may_change
        same = got[keep].view(np.uint64) == np.ascontiguousarray(psi[keep]).view(np.uint64)
        assert same.all(), (f"{np.count_nonzero(~same.reshape(-1, 2).all(axis=1))} amplitudes outside "
                            f"the circuit's subspace changed, first at index "
                            f"{np.flatnonzero(keep)[np.argmin(same.reshape(-1, 2).all(axis=1))]}")
    err = float(max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag))))
    if is_exact(info, jit) if exact is None else exact:
        assert err == 0.0 and np.array_equal(got, want), f"circuit of exact ops differs by {err:.3e}"
    else:
        assert err <= TOL, f"max component error {err:.3e} > {TOL:g}"
    return err


def generated_circuits(qsim, s):
    """The circuits configuration `s` runs through the generated kernels, as (label, gates, info):
    few, because each costs one hipRTC compile.  Candidates are the pooled circuits, then the
    steered cases on their own (pooling undoes their steering, so the pooled circuits alone miss
    required classes); a greedy cover picks, while any pattern of required(s) is uncovered, the
    candidate that covers the most of them (the first on ties).  Deterministic."""
    from qsim_amd import plan
    n = s["n"]
    cand = [(f"pooled{k}", gs) for k, gs in enumerate(pooled(s))]
    cand += [(label, gs) for label, gs, single in cases(s) if single is False]
    infos = [plan.plan_stage_info(circuit_of(qsim, n, gs)) for _, gs in cand]
    want = required(s)
    covers = [{i for i, p in enumerate(want) if any(matches(p, k) for k in classes_of(info))} for info in infos]
    left, picked = set(range(len(want))), []
    while left:
        best = max(range(len(cand)), key=lambda c: (len(covers[c] & left), -c))
        if not covers[best] & left:
            break  # (a required class no case reaches: the caller's coverage assertion reports it)
        picked.append(best)
        left -= covers[best]
    return [(cand[c][0], cand[c][1], infos[c]) for c in sorted(picked)]


def run_generated(qsim, s):
    """generated_circuits(s), each through fromHost -> run(c, Fused) -> toHost with the generated
    kernels (the caller set set_jit(2, 0)) against the dense reference; every staged pass of every
    circuit must have run as a generated kernel, so the classes counted are classes the generated
    source took.  Returns (circuits run, worst error, failure messages, classes hit, generated
    passes, generated passes of two or more stages)."""
    n = s["n"]
    sv = qsim.StateVector(n)
    ran, worst, failures, hit, jit_passes, multi = 0, 0.0, [], set(), 0, 0
    try:
        for k, (label, gates, info) in enumerate(generated_circuits(qsim, s)):
            psi = dense_state(n, 5000 * n + k)
            want, may = reference(n, psi, gates)
            sv.fromHost(psi)
            sv.run(circuit_of(qsim, n, gates), qsim.RunMode.Fused)
            jp = sv.lastRunInfo()[1]
            ran += 1
            try:
                staged = [p for p in info["passes"] if not p["single"] and p["rb"] > 0]
                assert jp == len(staged) >= 1, f"{jp} of {len(staged)} staged passes ran as generated kernels"
                worst = max(worst, check(sv.toHost(), psi, want, may, info, jit=True))
            except AssertionError as e:
                failures.append(f"{s['name']} {label}: {e}")
                break
            hit |= classes_of(info)
            jit_passes += jp
            multi += sum(p["stages"] >= 2 for p in staged)
    finally:
        sv.close()
    return ran, worst, failures, hit, jit_passes, multi


def relayout_circuit(n=16, seed=0, layers=5):
    """A circuit wider than one tile, so that a relayout plan exists for it (relayout.hip: from 16
    qubits) and its passes really move qubits: `layers` times a random one-qubit gate on every qubit,
    a random two-qubit gate on every pair of a random pairing, and one Toffoli."""
    rng = np.random.default_rng(900 + 17 * n + seed)
    gs = []
    for _ in range(layers):
        for q in range(n):
            t = int(rng.integers(X, RZ + 1))
            gs.append((t, [q], _angle(rng) if t >= RX else 0.0))
        perm = [int(q) for q in rng.permutation(n)]
        for a, b in zip(perm[::2], perm[1::2]):
            t = int(rng.choice([CNOT, CZ, CRY, CRZ, SWAP]))
            gs.append((t, [a, b], _angle(rng) if t in (CRY, CRZ) else 0.0))
        gs.append((TOFFOLI, [int(q) for q in rng.choice(n, 3, replace=False)], 0.0))
    return gs


def run_matrix(qsim, s, case_list=None, stop_at=6):
    """Every case of configuration `s` through StateVector.fromHost -> run(c, Fused) -> toHost
    under the settings in force (the caller applied them).  Returns (cases run, worst error,
    failure messages, classes hit)."""
    from qsim_amd import plan
    n = s["n"]
    case_list = cases(s) if case_list is None else case_list
    sv = qsim.StateVector(n)
    ran, worst, failures, hit = 0, 0.0, [], set()
    try:
        for k, (label, gates, single) in enumerate(case_list):
            if len(failures) >= stop_at:
                break
            c = circuit_of(qsim, n, gates)
            info = plan.plan_stage_info(c)
            hit |= classes_of(info)
            psi = dense_state(n, 1000 * n + k)
            want, may = reference(n, psi, gates)
            sv.fromHost(psi)
            sv.run(c, qsim.RunMode.Fused)
            ran += 1
            try:
                worst = max(worst, check(sv.toHost(), psi, want, may, info))
            except AssertionError as e:
                failures.append(f"{s['name']} {label}: {e}")
    finally:
        sv.close()
    return ran, worst, failures, hit
