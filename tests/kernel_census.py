#!/usr/bin/env python3
"""Which solver kernel a test reaches -- the rule, the universe and the table of holes (no device needed).

csrc/nmpc_capi.hip names the solver, evaluation and trace kernels in three switches (``solve_kernel_of``, ``eval_kernel_of``,
``trace_kernel_of``) over the ``Variant`` that csrc/nmpc_plan.h decides on. This module

* evaluates the plan header on the CPU (``Plan``: a few lines of C++ against nmpc_plan.h, built with g++ as tests/test_plan_cpu.py
  builds its own) for a configuration, an element size, a batch size, a device size and an entry (solve / eval / trace);
* restates the three switches in Python as the short names of tools/kernel_resources.py (``kernel_names``, ``trace_name``) and
  lists every name they can return (``universe``) -- tests/test_kernel_census_cpu.py holds that list against the kernels of the
  shipped code object, in both directions, which is also what proves the restated rule;
* lists the cases that the declared suites run (``declared``: built from THEIR case tables) and, one row per kernel that those
  do not name, the rows of ``CENSUS`` that tests/test_gpu_kernel_census.py runs on the device.

The pair member of a launch: 1 (axis-aligned path / compressed global table) with ``axis_aligned = 1``, or with
``axis_aligned = 0`` when no ellipse of the batch has a non-zero angle (the scan of the batch decides for the whole launch);
otherwise 2 (general path / general table). Flat or tail latency member: the plan's family.

    python tests/kernel_census.py            the universe, who names each kernel
    python tests/kernel_census.py --fuzz     how many calls of the fixed-seed fuzz runs of tests/test_gpu_fuzz.py reach each kernel
                                             (replayed on the CPU; the record is profiles/kernel_census_fuzz.txt)"""
import collections
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
CSRC = os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc")

# nmpc_plan::Family
THROUGHPUT, LATENCY_FLAT, LATENCY_TAIL, COOP, COOP_ONCHIP, EVAL, EVAL_COOP, EVAL_COOP_ONCHIP = range(8)
TRACE = 99          # (not a family of the plan: nmpc_solve_trace_f64 goes by the fp64 layout alone)
Variant = collections.namedtuple("Variant", "family lps glb rs hlp pair")
ENTRIES = ("solve", "eval", "trace")
# the options of nmpc_config that the plan reads, in the driver's order
OPTIONS = ("max_active_dynobs", "latency_waves", "coop_waves", "reg_table", "batch_invariant", "axis_aligned", "tail_latency", "staged")
SIMDS = (1024, 256)  # device sizes at which the census rows are held: an MI355X and a quarter of one

# one case per input line -> main variant | tail hand-off and its variant | dispatch order from one evaluation and its variant
DRIVER = r"""
#include <cstdio>
#include "nmpc_plan.h"
using namespace nmpc_plan;
static void put(const Variant& v) { printf("%d %d %d %d %d %d ", (int)v.family, v.lps, (int)v.glb, v.rs, (int)v.hlp, (int)v.pair); }
int main()
{
    int N, Nother, Nstc, Ndyn, hint, lw, cw, rt, bi, aa, tl, st, elem, B, n_simd, entry;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &N, &Nother, &Nstc, &Ndyn, &hint, &lw, &cw, &rt, &bi, &aa, &tl, &st, &elem, &B,
                 &n_simd, &entry) == 16) {
        nmpc_config c = {};
        c.N_hor = N, c.Nother = Nother, c.Nstcobs = Nstc, c.Ndynobs = Ndyn, c.max_active_dynobs = hint;
        c.latency_waves = lw, c.coop_waves = cw, c.reg_table = rt, c.batch_invariant = bi, c.axis_aligned = aa, c.tail_latency = tl, c.staged = st;
        c.max_outer_iterations = 6;
        const Layouts lays = make_layouts(c);
        const Layout& L = lays.main(elem);
        const PlanStatic s = {&c, &lays, (size_t)elem, n_simd, latency_fits(L, elem), coop_fits(L, elem)};
        const Variant none = {kThroughput, 0, false, 0, false, false};
        if (entry == 0) {
            const SolvePlan p = plan_solve(s, {B, false, true, true});
            put(p.main.variant);
            printf("%d ", (int)p.tail);
            put(p.tail ? p.tail_kernel.variant : none);
            printf("%d ", (int)p.eval_order);
            put(p.eval_order ? choose_single(s, kEval).variant : none);
        } else if (entry == 1) {
            put(plan_eval(s).variant);
            printf("0 "), put(none), printf("0 "), put(none);
        } else {
            const Variant t = {(Family)99, lays.lps, lays.lay64.glb, 0, false, false};
            put(t);
            printf("0 "), put(none), printf("0 "), put(none);
        }
        printf("\n");
    }
    return 0;
}
"""


class Plan:
    """The plan header on the CPU. ``Plan(directory)`` builds the driver there; ``plan(cases)`` -> per case the variants
    ``(main, tail or None, order or None)``. A case: ``(dims (N, Nother, Nstcobs, Ndynobs), options {name: value}, elem, B, S, entry)``."""

    def __init__(self, directory):
        src, self.exe = os.path.join(directory, "census_driver.cpp"), os.path.join(directory, "census_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", self.exe], check=True)

    def __call__(self, cases):
        lines = []
        for dims, options, elem, B, S, entry in cases:
            assert set(options) <= set(OPTIONS), options
            lines.append(" ".join(str(int(v)) for v in (*dims, *(options.get(k, 0) for k in OPTIONS), elem, B, S, ENTRIES.index(entry))))
        out = subprocess.run([self.exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        res = []
        for line in out:
            w = [int(x) for x in line.split()]
            var = lambda o: Variant(w[o], w[o + 1], bool(w[o + 2]), w[o + 3], bool(w[o + 4]), bool(w[o + 5]))
            res.append((var(0), var(7) if w[6] else None, var(14) if w[13] else None))
        return res


# ---- the three switches of csrc/nmpc_capi.hip, as short names ---------------------------------------------------------------------
def _b(x):
    return "true" if x else "false"


def _lps(lps):                       # with_lps
    return 3 if lps == 3 else 2 if lps == 2 else 1


def _slots(rs, elem):                # with_reg_slots: fp64 has the 14-slot table only
    return rs if elem == 4 and rs in (4, 6) else 14


def trace_name(lps, glb):
    """trace_kernel_of"""
    return f"trace_kernel<{_lps(lps)}, {_b(glb)}>"


def kernel_names(v, elem, member=1):
    """solve_kernel_of / eval_kernel_of (by the variant's family) and trace_kernel_of: the kernel of ``member`` (1 / 2) of the
    variant for ``elem`` = 4 / 8 bytes, as a tuple of one short name -- empty where the switch returns no kernel."""
    T = "float" if elem == 4 else "double"
    second = member == 2
    only = 2 if second else 1
    if v.family == TRACE:
        return (trace_name(v.lps, v.glb),) if elem == 8 and not second else ()
    if second and not v.pair:
        return ()
    if v.family == THROUGHPUT:
        if v.pair:
            return (f"solve_kernel<{T}, 3, false, {_slots(v.rs, elem)}, {only}>",)
        return (f"solve_kernel<{T}, {_lps(v.lps)}, {_b(v.glb)}, 0, 0>",)
    if v.family in (LATENCY_FLAT, LATENCY_TAIL):
        tail = v.family == LATENCY_TAIL
        if elem == 4 and v.pair:         # (the register-table members, and with them the tail members, exist in fp32 only)
            return (f"solve_spec_kernel<float, 3, false, {_slots(v.rs, elem)}, {only}, {_b(not tail)}>",)
        if tail:
            return ()
        return (f"solve_spec_kernel<{T}, {_lps(v.lps)}, {_b(v.glb)}, 0, 0, true>",)
    if v.family == COOP:
        return (f"solve_coop_kernel<{T}, {_lps(v.lps)}, {_b(v.glb)}, {0 if not v.glb else only}>",)
    if v.family == COOP_ONCHIP:
        return (f"solve_coop_reg_kernel<{_b(v.hlp)}>",) if elem == 4 else ()
    if v.family == EVAL:
        if v.pair:
            return (f"eval_kernel<{T}, 3, false, {_slots(v.rs, elem)}, {only}>",)
        return (f"eval_kernel<{T}, {_lps(v.lps)}, {_b(v.glb)}, 0, 0>",)
    if v.family == EVAL_COOP:
        return (f"eval_coop_kernel<{T}, {_lps(v.lps)}, {_b(v.glb)}, 0, false, 4, {0 if not v.glb else only}>",)
    if v.family == EVAL_COOP_ONCHIP:
        return (f"eval_coop_kernel<float, 1, false, 12, {_b(v.hlp)}, 8, 0>",) if elem == 4 else ()
    return ()


def member_of(axis_aligned, rotated):
    """The pair member that does the work of a launch (KParams::axis_mode; the other one returns at once)."""
    return 1 if axis_aligned > 0 or (axis_aligned == 0 and not rotated) else 2


def _variants():
    """Every Variant that the constructors of nmpc_plan.h build (single_variant over the main and the fp64 register-table layouts,
    coop_variant, coop_onchip_variant), per element size: a register table means three lanes per step and no global table
    (make_layout), 4 / 6 / 14 slots in fp32 and 14 in fp64, where only the throughput and the evaluation family take it
    (choose_reg64); and the trace entry's (lps, glb)."""
    for elem in (4, 8):
        for lps in (1, 2, 3):
            for glb in (False, True):
                for f in (THROUGHPUT, LATENCY_FLAT, LATENCY_TAIL, EVAL):
                    yield Variant(f, lps, glb, 0, False, False), elem
                for f in (COOP, EVAL_COOP):
                    yield Variant(f, lps, glb, 0, False, glb), elem
                if elem == 8:
                    yield Variant(TRACE, lps, glb, 0, False, False), elem
        for rs in ((4, 6, 14) if elem == 4 else (14,)):
            for f in ((THROUGHPUT, LATENCY_FLAT, LATENCY_TAIL, EVAL) if elem == 4 else (THROUGHPUT, EVAL)):
                yield Variant(f, 3, False, rs, False, True), elem
        for hlp in (False, True):
            for f in (COOP_ONCHIP, EVAL_COOP_ONCHIP):
                yield Variant(f, 1, False, 12, hlp, False), elem


@functools.lru_cache(maxsize=None)
def universe():
    """name -> (variant, elem, member) of every kernel that the switches return for a variant of the plan."""
    names = {}
    for v, elem in _variants():
        for member in (1, 2):
            for n in kernel_names(v, elem, member):
                names.setdefault(n, (v, elem, member))
    return names


# ---- what a case reaches ------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "id entry elem dims options B rotated")


def reached(plan, cases, S):
    """Per case the set of kernels that its call runs on a device of ``S`` SIMDs: the main kernel, the tail member where the plan
    hands off and the evaluation kernel where it takes the dispatch order from one evaluation."""
    out = []
    for c, (main, tail, order) in zip(cases, plan([(c.dims, c.options, c.elem, c.B, S, c.entry) for c in cases])):
        m = member_of(c.options.get("axis_aligned", 0), c.rotated)
        names = set()
        for v in (main, tail, order):
            if v is not None:
                names.update(kernel_names(v, c.elem, m if v.pair else 1))
        out.append(names)
    return out


def _rotated(P, lay):
    return bool(np.asarray(P)[:, lay.od:lay.od + 6 * (lay.N + 1) * lay.Ndyn].reshape(-1, 6)[:, 4].any())


@functools.lru_cache(maxsize=None)
def declared():
    """The cases of the declared suites, from their own tables: CASES of test_gpu_fp32_paths.py, CASES x (evaluation: both
    reg_table settings; solves: MODES) of test_gpu_dims_sweep.py, DIMS x (evaluation; KERNELS) of test_gpu_read_bounds.py, in both
    precisions where the suite runs both, each with the axis-alignment of the batch that the file itself makes.
    Left out: what does not fix its kernel by its configuration alone -- latency_waves = 0 or coop_waves = 0 in a solve (the
    "automatic" mode of the dims sweep: the plan goes by the batch size and the device's SIMD count), and with them the suites that
    run on the automatic plan throughout (parity, plan / warm start, tail, capacity, closed loop). The parity / coop / history /
    off-nominal cases with a global table all have N = 40, one lane per step, like "tp-glb" and the N = 40 rows here."""
    import dyobav_mpcnwta_warehouse_amd as nm
    import test_gpu_dims_sweep as sweep
    import test_gpu_fp32_paths as paths
    import test_gpu_read_bounds as bounds
    cases = []
    for cid, (N, Ndyn, hint, rows, per, rotate, ov, _) in paths.CASES.items():
        lay = nm.scenarios.ParamLayout(N, 10, 10, Ndyn)
        opt = {k: v for k, v in ov.items() if k in OPTIONS}
        opt["max_active_dynobs"] = hint
        cases.append(Case(f"fp32_paths/{cid}", "solve", 4, (N, 10, 10, Ndyn), opt, 5 * per, _rotated(paths._batch(N, Ndyn, rows, per, rotate), lay)))
    for dims in sweep.CASES:
        # the batches as the file's two tests build them: K = 6, seed 100 for the evaluations; K = 8, seed 200 for the solves
        lay, Pe = sweep._batch(6, 100, *dims)
        _, Ps = sweep._batch(8, 200, *dims)
        d, rot_e, rot = (lay.N, lay.Nother, lay.Nstc, lay.Ndyn), _rotated(Pe, lay), _rotated(Ps, lay)
        for elem in (8, 4):
            for rt in sweep.EVAL_REG_TABLES:
                cases.append(Case(f"dims_sweep/eval-N{d[0]}-dyn{d[3]}-rt{rt}-f{8 * elem}", "eval", elem, d, dict(reg_table=rt), 6, rot_e))
            for name, ov in sweep.MODES:
                cases.append(Case(f"dims_sweep/{name}-N{d[0]}-dyn{d[3]}-f{8 * elem}", "solve", elem, d, dict(ov), 8, rot))
    for dims in bounds.DIMS:
        lay, _, P, _, _, _ = bounds._problem(*dims)
        d, rot = (lay.N, lay.Nother, lay.Nstc, lay.Ndyn), _rotated(P, lay)
        for elem in (8, 4):
            cases.append(Case(f"read_bounds/eval-N{d[0]}-dyn{d[3]}-f{8 * elem}", "eval", elem, d, {}, P.shape[0], rot))
            for name, ov in bounds.KERNELS.items():
                cases.append(Case(f"read_bounds/{name}-N{d[0]}-dyn{d[3]}-f{8 * elem}", "solve", elem, d, dict(ov), P.shape[0], rot))
    return tuple(c for c in cases if c.entry != "solve" or (c.options.get("latency_waves", 0) != 0 and c.options.get("coop_waves", 0) != 0))


def declared_names(plan):
    """name -> ids of the declared cases that reach it (the main kernel of the case: with both wave counts given it is the same on
    every device; asserted for the sizes of SIMDS)."""
    cases = declared()
    per_size = [[sorted(kernel_names(main, c.elem, member_of(c.options.get("axis_aligned", 0), c.rotated) if main.pair else 1))
                 for c, (main, _, _) in zip(cases, plan([(c.dims, c.options, c.elem, c.B, S, c.entry) for c in cases]))] for S in SIMDS]
    assert all(p == per_size[0] for p in per_size[1:])
    names = {}
    for c, ns in zip(cases, per_size[0]):
        assert ns, c
        for n in ns:
            names.setdefault(n, []).append(c.id)
    return names


# ---- the holes: one row per kernel that no declared case names -------------------------------------------------------------------------
# A row: id, entry, element size, (N, Nother, Nstcobs, Ndynobs), nmpc_config overrides (both wave counts given, never 0: the kernel
# then does not depend on the device's size), whether every other instance of the batch is turned, the kernel the row must
# reach, and its obstacles: eval rows -- the number of provisioned rows that hold an obstacle on the robot's path (B = 3, as
# _problem of test_gpu_read_bounds.py); solve and trace rows -- (pedestrians, hypotheses each) of the batch of
# test_gpu_fp32_paths._batch, 8 instances per family. A quarter to a half of the provisioned rows are occupied, so that soft and
# hard terms are both active.
Row = collections.namedtuple("Row", "id entry elem dims options rotated kernel obstacles")
EVAL_B = 3
PER_FAMILY = 8


@functools.lru_cache(maxsize=None)
def first_global(N, elem):
    """The smallest Ndynobs (Nother = Nstcobs = 10, no hint) whose obstacle table nmpc_layout places in the global workspace."""
    import dyobav_mpcnwta_warehouse_amd as nm
    for Ndyn in range(1, 2000):
        cfg = nm.default_config_struct()
        cfg.N_hor, cfg.Nother, cfg.Nstcobs, cfg.Ndynobs = N, 10, 10, Ndyn
        li = nm.layout_info(cfg)
        if (li.global_table_f32 if elem == 4 else li.global_table_f64):
            return Ndyn
    raise AssertionError((N, elem))


def _peds(Ndyn):
    """(pedestrians, hypotheses each) that occupy a quarter to a half of Ndyn rows."""
    n_hyp = max(1, min(20, Ndyn // 8))
    n_ped = max(1, (3 * Ndyn // 8) // n_hyp)
    assert Ndyn < 4 or Ndyn / 4 <= n_ped * n_hyp <= Ndyn / 2, (Ndyn, n_ped, n_hyp)
    return n_ped, n_hyp


def _census():
    rows, boundary = [], []
    ONE = dict(latency_waves=1, coop_waves=1)            # one wavefront per instance: the throughput family
    AX, GEN = dict(axis_aligned=1), dict(axis_aligned=-1)

    def add(to, rid, entry, elem, N, Ndyn, opt, rot, kernel):
        obst = 3 * Ndyn // 8 if entry == "eval" else _peds(Ndyn)
        to.append(Row(f"{rid}-f{8 * elem}", entry, elem, (N, 10, 10, Ndyn), opt, rot, kernel, obst))

    for elem, T in ((8, "double"), (4, "float")):
        g = {3: (21, first_global(21, elem)), 2: (32, first_global(32, elem)), 1: (33, first_global(33, elem))}
        lds = {3: (20, 15), 2: (32, 20), 1: (40, 24)}
        # -- evaluations: the streamed table at three and two lanes per step, and the LDS side of each boundary
        for l in (3, 2):
            N, Ndyn = g[l]
            add(rows, f"eval-glb-l{l}", "eval", elem, N, Ndyn, dict(ONE), False, f"eval_kernel<{T}, {l}, true, 0, 0>")
            add(boundary, f"eval-lds-l{l}-below-glb", "eval", elem, N, Ndyn - 1, dict(ONE), False, f"eval_kernel<{T}, {l}, false, 0, 0>")
        # -- the cooperative kernels' evaluation: LDS table, then both members of the global-table pair, per lane map
        for l in (3, 2, 1):
            N, Ndyn = lds[l]
            add(rows, f"evalcoop-lds-l{l}", "eval", elem, N, Ndyn, dict(latency_waves=1, coop_waves=4, reg_table=-1), True,
                f"eval_coop_kernel<{T}, {l}, false, 0, false, 4, 0>")
            N, Ndyn = g[l]
            add(rows, f"evalcoop-glb-l{l}-compressed", "eval", elem, N, Ndyn, dict(latency_waves=1, coop_waves=4, reg_table=-1, **AX), False,
                f"eval_coop_kernel<{T}, {l}, true, 0, false, 4, 1>")
            add(rows, f"evalcoop-glb-l{l}-general", "eval", elem, N, Ndyn, dict(latency_waves=1, coop_waves=2, reg_table=-1, **GEN), True,
                f"eval_coop_kernel<{T}, {l}, true, 0, false, 4, 2>")
        # -- the general members of the register-table evaluation (full tables: every slot holds a row)
        for slots, Ndyn in ((4, 12), (6, 18), (14, 42)) if elem == 4 else ((14, 42),):
            add(rows, f"eval-reg{slots}-general", "eval", elem, 20, Ndyn, dict(ONE, reg_table=0 if elem == 4 else 1, **GEN), True,
                f"eval_kernel<{T}, 3, false, {slots}, 2>")
    # -- the on-chip cooperative evaluation: without helper lanes (N = 43) and with them (N = 33), one row beyond the registers
    add(rows, "evalcoop-onchip-n43", "eval", 4, 43, 97, dict(latency_waves=1, coop_waves=4, reg_table=0), True, "eval_coop_kernel<float, 1, false, 12, false, 8, 0>")
    add(rows, "evalcoop-onchip-n33-helpers", "eval", 4, 33, 145, dict(latency_waves=1, coop_waves=4, reg_table=0), True, "eval_coop_kernel<float, 1, false, 12, true, 8, 0>")

    for elem, T in ((8, "double"), (4, "float")):
        g = {3: (21, first_global(21, elem)), 2: (32, first_global(32, elem)), 1: (33, first_global(33, elem))}
        # -- solves on the streamed table at three and two lanes per step: throughput, latency, both cooperative members
        for l in (3, 2):
            N, Ndyn = g[l]
            add(rows, f"tp-glb-l{l}", "solve", elem, N, Ndyn, dict(ONE), True, f"solve_kernel<{T}, {l}, true, 0, 0>")
            add(rows, f"lat4-glb-l{l}", "solve", elem, N, Ndyn, dict(latency_waves=4, coop_waves=1), True, f"solve_spec_kernel<{T}, {l}, true, 0, 0, true>")
            add(rows, f"coop4-glb-l{l}-compressed", "solve", elem, N, Ndyn, dict(latency_waves=1, coop_waves=4, **AX), False,
                f"solve_coop_kernel<{T}, {l}, true, 1>")
            add(rows, f"coop2-glb-l{l}-general", "solve", elem, N, Ndyn, dict(latency_waves=1, coop_waves=2, **GEN), True,
                f"solve_coop_kernel<{T}, {l}, true, 2>")
    N, Ndyn = 33, first_global(33, 8)
    add(rows, "coop2-glb-l1-general", "solve", 8, N, Ndyn, dict(latency_waves=1, coop_waves=2, **GEN), True, "solve_coop_kernel<double, 1, true, 2>")
    # -- the fp64 register-table kernel (reg_table = 1 asks for it), both members
    add(rows, "tp-reg64-axis", "solve", 8, 20, 42, dict(ONE, reg_table=1, **AX), False, "solve_kernel<double, 3, false, 14, 1>")
    add(rows, "tp-reg64-general", "solve", 8, 20, 42, dict(ONE, reg_table=1, **GEN), True, "solve_kernel<double, 3, false, 14, 2>")
    # -- fp32 latency members that no declared case names: flat general members, tail members
    LAT = dict(latency_waves=4, coop_waves=1)
    add(rows, "lat4-reg14-flat-general", "solve", 4, 20, 42, dict(LAT, batch_invariant=-1, **GEN), True, "solve_spec_kernel<float, 3, false, 14, 2, true>")
    add(rows, "lat4-reg4-flat-general", "solve", 4, 20, 12, dict(LAT, batch_invariant=-1, **GEN), True, "solve_spec_kernel<float, 3, false, 4, 2, true>")
    add(rows, "lat4-reg4-tail-axis", "solve", 4, 20, 12, dict(LAT, batch_invariant=1, **AX), False, "solve_spec_kernel<float, 3, false, 4, 1, false>")
    add(rows, "lat4-reg4-tail-general", "solve", 4, 20, 12, dict(LAT, batch_invariant=1, **GEN), True, "solve_spec_kernel<float, 3, false, 4, 2, false>")
    add(rows, "lat4-reg6-tail-general", "solve", 4, 20, 18, dict(LAT, batch_invariant=1, **GEN), True, "solve_spec_kernel<float, 3, false, 6, 2, false>")
    # -- nmpc_solve_trace_f64: every lane map on both sides of the fp64 global-table boundary
    for l, N in ((3, 21), (2, 32), (1, 33)):
        Ndyn = first_global(N, 8)
        add(rows, f"trace-l{l}-glb", "trace", 8, N, Ndyn, dict(ONE), False, f"trace_kernel<{l}, true>")
        add(rows, f"trace-l{l}-lds", "trace", 8, N, Ndyn - 1, dict(ONE), False, f"trace_kernel<{l}, false>")
    order = {e: i for i, e in enumerate(ENTRIES)}
    order["solve"], order["eval"] = 1, 0                     # the file order of the device test: eval, solve, trace
    rows.sort(key=lambda r: order[r.entry])
    return tuple(rows), tuple(boundary)


@functools.lru_cache(maxsize=None)
def census():
    """(CENSUS, BOUNDARY): the rows need nmpc_layout, i.e. the built library, so they are made on first use."""
    return _census()


def __getattr__(name):          # kernel_census.DECLARED, .CENSUS, .BOUNDARY: the tables of declared() and census()
    if name == "DECLARED":
        return declared()
    if name in ("CENSUS", "BOUNDARY"):
        return census()[("CENSUS", "BOUNDARY").index(name)]
    raise AttributeError(name)


def row_case(r, B=None):
    """The row as a Case of `reached` (B: 3 for evaluations, 8 per family for solves, 1 for a trace)."""
    B = B or {"eval": EVAL_B, "solve": 5 * PER_FAMILY, "trace": 1}[r.entry]
    return Case(r.id, r.entry, r.elem, r.dims, r.options, B, r.rotated)


def coverage(plan, rows, names=None):
    """(kernels of the universe that neither a declared case nor a row names, rows whose kernel a declared case names already)."""
    names = declared_names(plan) if names is None else names
    by_row = {r.id: r.kernel for r in rows}
    unnamed = sorted(set(universe()) - set(names) - set(by_row.values()))
    twice = sorted(rid for rid, k in by_row.items() if k in names)
    return unnamed, twice


# ---- the batches of the rows ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def eval_problem(dims, n_rows, rotated):
    """B = 3 instances with `n_rows` of the provisioned obstacle rows ON the robot's path (as fuzz_eval.make_case places them: soft
    and hard ellipse terms both active, rx != ry, half of the rows dealt into groups that share their t = 0 snapshot -- the
    kernels merge those), a point to evaluate at, multipliers and penalties as _problem of test_gpu_read_bounds.py.
    `rotated`: the ellipses of every other instance are turned. Returns (lay, P, U, Y, C); shared by the rows of the same dimensions."""
    import dyobav_mpcnwta_warehouse_amd as nm
    N, Nother, Nstc, Ndyn = dims
    lay = nm.scenarios.ParamLayout(N=N, Nother=Nother, Nstc=Nstc, Ndyn=Ndyn)
    B = EVAL_B
    rng = np.random.default_rng(7000 + 1000 * N + Ndyn)
    P = nm.scenarios.make_batch(B, lay, seed=300 + N + Ndyn, n_ped=0, n_hyp=1, n_boxes=4, ped_mode="oncoming")
    s0 = P[:, lay.s0:lay.s0 + 3]
    ref = P[:, lay.rs:lay.rs + 3 * N].reshape(B, N, 3)
    od = np.zeros((B, Ndyn, N + 1, 6))
    slots = rng.permutation(Ndyn)[:n_rows]
    for b in range(B):
        path = np.r_[s0[b:b + 1, :2], ref[b, :, :2]]
        for j in slots:
            ctr = path[rng.integers(0, N)] + rng.normal(0, 0.3, 2)
            od[b, j, :, 0:2] = ctr + np.arange(N + 1)[:, None] * rng.normal(0, 0.03, 2)
            od[b, j, :, 2] = rng.uniform(0.2, 0.9)
            od[b, j, :, 3] = od[b, j, :, 2] * rng.choice([0.6, 1.5])                    # rx != ry
            od[b, j, :, 4] = rng.uniform(-1.2, 1.2) if rotated and b % 2 == 0 else 0.0
            od[b, j, :, 5] = rng.uniform(0.0, 1.0, N + 1)
    n_groups = max(1, n_rows // 4)
    for j in slots[n_groups:n_groups + n_rows // 2]:
        od[:, j, 0, 0:5] = od[:, slots[int(rng.integers(0, n_groups))], 0, 0:5]
    P[:, lay.od:lay.od + od[0].size] = od.reshape(B, -1)
    assert _rotated(P, lay) == rotated
    U = np.stack([rng.uniform(-0.3, 1.4, (B, N)), rng.uniform(-0.45, 0.45, (B, N))], axis=2).reshape(B, 2 * N)
    Y = rng.normal(size=(B, 2 * N)) * 2
    C = rng.uniform(1, 200, B)
    return lay, P, U, Y, C


def solve_batch(dims, peds, rotated):
    """8 instances of each family of test_gpu_fp32_paths.py (its _batch: pedestrians on the robot's path, rx != ry, every other
    instance turned if `rotated`), float32 values; the rows' weights, 1 there, drawn from 0.3 .. 1 per row and step here, so that
    a weight that a kernel drops or misplaces shows."""
    return _solve_batch(tuple(dims), tuple(peds), bool(rotated))


@functools.lru_cache(maxsize=None)
def _solve_batch(dims, peds, rotated):
    import dyobav_mpcnwta_warehouse_amd as nm
    import test_gpu_fp32_paths as paths
    N, Nother, Nstc, Ndyn = dims
    assert (Nother, Nstc) == (10, 10)
    lay = nm.scenarios.ParamLayout(N, Nother, Nstc, Ndyn)
    P = paths._batch(N, Ndyn, peds, PER_FAMILY, rotated).copy()
    od = P[:, lay.od:lay.od + 6 * (N + 1) * Ndyn].reshape(P.shape[0], Ndyn, N + 1, 6)
    od[..., 5] *= np.random.default_rng(500 + N + Ndyn).uniform(0.3, 1.0, od[..., 5].shape).astype(np.float32)
    P.setflags(write=False)
    return P


# ---- the fixed-seed fuzz runs, replayed on the CPU ------------------------------------------------------------------------------------------
def fuzz_report(plan, out=print, S=SIMDS[0]):
    """How many calls of the fuzz runs of tests/test_gpu_fuzz.py reach each kernel of the universe: make_case with their seeds and
    case counts, the modes of fuzz_eval.run and fuzz_solve.run, the plan at `S` SIMDs (the "automatic" mode of the solves goes by it).
    A record, not a condition: returns {kernel: {run: calls}}."""
    import fuzz_eval
    import fuzz_solve
    import test_gpu_fuzz as tf
    runs = [(f"eval seed {s}", "eval", s, tf.EVAL_CASES, None) for s in tf.EVAL_SEEDS]
    runs += [(f"solve f64 seed {s}", "solve", s, n, 8) for s, _, _, n in tf.SOLVE_RUNS]
    runs += [(f"solve f32 seed {s}", "solve", s, tf.SOLVE_F32_CASES, 4) for s in tf.SOLVE_F32_SEEDS]
    counts = {k: collections.Counter() for k in universe()}
    for name, entry, seed, n, elem in runs:
        rng = np.random.default_rng(seed)
        cases = []
        for ci in range(n):
            lay, _, P, _, _, _ = fuzz_eval.make_case(rng)
            dims, rot = (lay.N, lay.Nother, lay.Nstc, lay.Ndyn), _rotated(P, lay)
            if entry == "eval":
                for e in (8, 4):
                    cases += [Case(mode, "eval", e, dims, dict({k: v for k, v in ov.items() if k in OPTIONS}, latency_waves=1), P.shape[0], rot)
                              for mode, ov in fuzz_eval.eval_modes(ci)]
            else:
                cases += [Case(mode, "solve", elem, dims, {k: v for k, v in ov.items() if k in OPTIONS}, P.shape[0], rot)
                          for mode, ov in fuzz_solve._modes(ci, elem == 4, not rot)]
        for names in reached(plan, cases, S):
            for k in names:
                counts[k][name.split(" seed")[0]] += 1
    cols = ("eval", "solve f64", "solve f32")
    out(f"calls of the fixed-seed fuzz runs of tests/test_gpu_fuzz.py per kernel (plan at {S} SIMDs); {sum(1 for c in counts.values() if not c)} of "
        f"{len(counts)} kernels are reached by none")
    out(f"{'kernel':58s} " + " ".join(f"{c:>10s}" for c in cols))
    for k in sorted(counts):
        out(f"{k:58s} " + " ".join(f"{counts[k][c]:10d}" for c in cols))
    return counts


def main(argv):
    with tempfile.TemporaryDirectory() as td:
        plan = Plan(td)
        if "--fuzz" in argv:
            fuzz_report(plan)
            return 0
        names = declared_names(plan)
        by_row = {r.kernel: r.id for r in census()[0]}
        print(f"{len(universe())} kernels; {len(names)} named by the {len(declared())} declared cases, {len(by_row)} by a census row")
        for k in sorted(universe()):
            print(f"{k:58s} {by_row.get(k) or names.get(k, ['-- NOT NAMED --'])[0]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
