"""CPU test: every solver kernel of the shipped code object is reached by a test that says so.

tests/kernel_census.py restates the three kernel switches of csrc/nmpc_capi.hip as names, lists every name they can give (the
universe), the cases of the declared suites and the rows of CENSUS that tests/test_gpu_kernel_census.py runs. Here:
  * the solver kernels of the shipped code object ARE the universe, in both directions (a wrong naming rule gives names that do
    not exist; a new instantiation is a name that no variant gives);
  * every kernel of the universe is named by a declared case or a CENSUS row, every row reaches the kernel it states (the plan
    header evaluated for 1 024 and for 256 SIMDs), and no row repeats what a declared case names already;
  * controls: without any one row the coverage check names the row's kernel; with axis_aligned flipped a pair row is reported
    on the other member.
A new instantiation fails the first test until the switches' restatement knows it, and the second until a row names it."""
import os
import re
import sys

import pytest

import dyobav_mpcnwta_warehouse_amd as nm
import kernel_census as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SOLVER_KERNELS = r"^(solve_kernel|solve_spec_kernel|solve_coop_kernel|solve_coop_reg_kernel|eval_kernel|eval_coop_kernel|trace_kernel)<"
# compiled solver kernels that no variant of the plan names, each with its reason (none today)
UNNAMED_BY_DESIGN = {}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return kc.Plan(str(tmp_path_factory.mktemp("census")))


@pytest.fixture(scope="module")
def compiled():
    import kernel_resources
    nm.build_library()
    names = {kernel_resources.short_name(k) for k in kernel_resources.kernel_resources(nm.library_path())}
    return {n for n in names if re.search(SOLVER_KERNELS, n)}


def test_the_compiled_solver_kernels_are_the_universe(compiled):
    universe = set(kc.universe())
    assert len(universe) == 110 and len(kc.CENSUS) + 52 == 110      # (the figures of DESIGN.md section 3)
    assert not universe - compiled, ("variants without a kernel", sorted(universe - compiled))
    assert compiled - universe == set(UNNAMED_BY_DESIGN), ("kernels that no variant names", sorted(compiled - universe))
    # every family of the switches is there, in both precisions where it exists
    for pattern in (r"^solve_kernel<double", r"^solve_spec_kernel<float, 3, false, 6, 2, false>", r"^solve_coop_reg_kernel<true>",
                    r"^eval_coop_kernel<float, 1, false, 12, true, 8, 0>", r"^trace_kernel<3, true>"):
        assert any(re.search(pattern, n) for n in universe), pattern


def test_every_kernel_is_named_by_a_declared_case_or_a_census_row(plan):
    names = kc.declared_names(plan)
    assert len(kc.declared()) > 200 and set(names) <= set(kc.universe())
    assert len(names) == 52
    unnamed, twice = kc.coverage(plan, kc.CENSUS, names)
    assert not unnamed, ("kernels that no declared case and no census row names", unnamed)
    assert not twice, ("census rows whose kernel a declared case names already", twice)
    assert len({r.id for r in kc.CENSUS + kc.BOUNDARY}) == len(kc.CENSUS) + len(kc.BOUNDARY)
    assert len({r.kernel for r in kc.CENSUS}) == len(kc.CENSUS)          # one row per kernel


def test_the_declared_suites_alone_leave_the_holes_that_the_issue_names(plan):
    unnamed, _ = kc.coverage(plan, ())
    assert set(unnamed) == {r.kernel for r in kc.CENSUS}
    # the fp32 global-table solve kernels at three lanes per step, which not even the fixed-seed fuzz runs reach
    assert {"solve_kernel<float, 3, true, 0, 0>", "solve_spec_kernel<float, 3, true, 0, 0, true>", "solve_coop_kernel<float, 3, true, 1>",
            "solve_coop_kernel<float, 3, true, 2>"} <= set(unnamed)
    # ... and every GLB instantiation at two and three lanes per step: 2 types x 2 lane maps x 7
    glb = [k for k in unnamed if re.search(r"^(solve_kernel|solve_spec_kernel|solve_coop_kernel|eval_kernel|eval_coop_kernel)<(float|double), [23], true", k)]
    assert len(glb) == 28, glb


@pytest.mark.parametrize("S", kc.SIMDS)
def test_every_census_row_reaches_the_kernel_it_states(plan, S):
    rows = kc.CENSUS + kc.BOUNDARY
    for r in rows:
        assert r.entry in kc.ENTRIES and r.kernel in kc.universe(), r
        assert r.options.get("latency_waves", 0) != 0 and r.options.get("coop_waves", 0) != 0, r      # never left to the device's size
        assert r.options.get("axis_aligned", 0) != 0 or not kc.universe()[r.kernel][0].pair, r        # a pair row pins its member
    for r, got in zip(rows, kc.reached(plan, [kc.row_case(r) for r in rows], S)):
        assert got == {r.kernel}, (S, r.id, sorted(got))
    # the order of the device test's file: evaluations, then solves, then traces
    entries = [r.entry for r in kc.CENSUS]
    assert entries == sorted(entries, key=("eval", "solve", "trace").index)


def test_the_boundary_rows_sit_one_row_below_the_global_table():
    """nmpc_layout on both sides: the streamed-table rows are the first Ndynobs with a global table, the boundary rows the last
    with the table in LDS (the numbers come from nmpc_layout, nothing here states them)."""
    glb = {(r.dims, r.elem) for r in kc.CENSUS if ", true" in r.kernel and not r.kernel.startswith(("solve_coop_reg", "eval_coop_kernel<float, 1, false, 12"))
           and re.search(r"<(float|double), \d, true|trace_kernel<\d, true", r.kernel)}
    assert len(glb) == 6
    for dims, elem in glb:
        for d, want in ((0, 1), (-1, 0)):
            cfg = nm.default_config_struct()
            cfg.N_hor, cfg.Nother, cfg.Nstcobs, cfg.Ndynobs = dims[0], dims[1], dims[2], dims[3] + d
            li = nm.layout_info(cfg)
            assert (li.global_table_f32 if elem == 4 else li.global_table_f64) == want, (dims, elem, d)
    for r in kc.BOUNDARY:
        assert ((r.dims[0], 10, 10, r.dims[3] + 1), r.elem) in glb and ", false" in r.kernel, r


def test_control_without_a_row_the_coverage_check_names_its_kernel(plan):
    names = kc.declared_names(plan)
    for i, r in enumerate(kc.CENSUS):
        unnamed, _ = kc.coverage(plan, kc.CENSUS[:i] + kc.CENSUS[i + 1:], names)
        assert unnamed == [r.kernel], (r.id, unnamed)


def test_control_a_flipped_axis_aligned_reaches_the_other_member(plan):
    pairs = [r for r in kc.CENSUS if kc.universe()[r.kernel][0].pair]
    assert len(pairs) >= 20
    flipped = [r._replace(options=dict(r.options, axis_aligned=-r.options["axis_aligned"])) for r in pairs]
    for r, got in zip(pairs, kc.reached(plan, [kc.row_case(f) for f in flipped], kc.SIMDS[0])):
        v, elem, member = kc.universe()[r.kernel]
        assert got == set(kc.kernel_names(v, elem, 3 - member)) and r.kernel not in got, (r.id, got)
    # axis_aligned = 0: the batch decides -- a turned batch goes to the general member, an axis-aligned one to the other
    for r in pairs[:4]:
        v, elem, _ = kc.universe()[r.kernel]
        auto = kc.row_case(r)._replace(options=dict(r.options, axis_aligned=0))
        for rot, member in ((False, 1), (True, 2)):
            assert kc.reached(plan, [auto._replace(rotated=rot)], kc.SIMDS[0])[0] == set(kc.kernel_names(v, elem, member))
