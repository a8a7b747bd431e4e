"""CPU tests of the fused network end's host side: ``mmp_stem.fold_head`` / ``check_head`` against a small module written anew
with the reference's attribute names, every refusal, the layout of the argument struct against the C compiler, the resources of
the shipped kernel, and the controls of the float64 restatement's bound (tests/mmp_head_reference.py) before any device run."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_head_reference as hr
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.mmp_stem import HEAD_FEATURES, HeadSpec, check_head, fold_head, head_features
from test_mmp_block2_cpu import ROOT

WRONG = ("ceil", "order", "sum", "slope")


class _Swarm(torch.nn.Module):
    def __init__(self, O, bias=True):
        super().__init__()
        self.layer_hypos = torch.nn.Linear(128, O, bias=bias)

    def forward(self, x):
        return self.layer_hypos(x)


class _End(torch.nn.Module):
    """The end of the reference's ConvMultiHypoNet(lite=True) by its attribute names, written anew."""
    def __init__(self, C, H, W, O, bias=True):
        super().__init__()
        nn = torch.nn
        torch.manual_seed(100 * C + O)
        self.apool = nn.AvgPool2d(2, 2)
        self.fc1, self.leaky, self.swarm = nn.Linear(head_features(C, H, W), 128, bias=bias), nn.LeakyReLU(0.01), _Swarm(O, bias)

    def forward(self, x):
        x = self.apool(x)
        return self.swarm(self.leaky(self.fc1(x.view(x.size(0), -1))))


# ---- 1. the fold ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W,O,bias", [(8, 3, 3, 2, True), (16, 4, 7, 40, True), (128, 10, 11, 40, False)], ids=["odd", "wide", "warehouse-no-bias"])
def test_fold_equals_the_module_in_float64(C, H, W, O, bias):
    end = _End(C, H, W, O, bias).eval()
    spec = fold_head(end.apool, end.fc1, end.leaky, end.swarm)
    assert isinstance(spec, HeadSpec) and spec.slope == pytest.approx(0.01) and HEAD_FEATURES == hr.FEATURES == 128
    assert spec.w1.shape == (128, hr.features(C, H, W)) and spec.c1.shape == (128,) and spec.w2.shape == (O, 128) and spec.c2.shape == (O,)
    assert all(v.dtype == np.float32 and v.flags.c_contiguous for v in spec if isinstance(v, np.ndarray))
    assert bias == bool(np.abs(spec.c1).max() > 0) == bool(np.abs(spec.c2).max() > 0)              # a missing bias folds to zeros
    x = hr.random_x(3, C, H, W, seed=5)
    end.double()
    with torch.no_grad():
        want = end(torch.from_numpy(x).double()).numpy()
    got, bound = hr.head(x, spec)                              # (the module's parameters are float32 values: the fold rounds nothing)
    print(f"{C} x {H} x {W} -> {O}: largest |restatement - module| = {np.abs(got - want).max():.2e}")
    assert got.shape == want.shape == (3, O) and np.abs(got - want).max() <= 1e-12 and (bound > 0).all()
    # a plain Linear as the swarm is taken as well
    plain = fold_head(end.apool, end.fc1.float(), end.leaky, end.swarm.layer_hypos.float())
    assert np.array_equal(plain.w2, spec.w2) and np.array_equal(plain.c2, spec.c2)


# ---- 2. the refusals --------------------------------------------------------------------------------------------------------------------------
def test_fold_refuses_what_the_kernel_does_not_compute():
    nn = torch.nn
    end = _End(16, 4, 7, 40).eval()
    good = dict(apool=end.apool, fc1=end.fc1, leaky=end.leaky, swarm=end.swarm)
    fold_head(**good)
    for match, over in [
            ("'apool' must be AvgPool2d\\(2, 2\\)", dict(apool=nn.AvgPool2d(3, 2))),
            ("'apool' must be AvgPool2d\\(2, 2\\)", dict(apool=nn.AvgPool2d(2, 1))),
            ("'apool' must be AvgPool2d\\(2, 2\\)", dict(apool=nn.AvgPool2d(2, 2, padding=1))),
            ("'apool' must be AvgPool2d\\(2, 2\\)", dict(apool=nn.AvgPool2d(2, 2, ceil_mode=True))),
            ("'apool' must be AvgPool2d\\(2, 2\\)", dict(apool=nn.AvgPool2d(2, 2, divisor_override=3))),
            ("'apool' must be AvgPool2d\\(2, 2\\)", dict(apool=nn.MaxPool2d(2, 2))),
            ("'apool' must be AvgPool2d\\(2, 2\\)", dict(apool=nn.AdaptiveAvgPool2d(2))),
            ("'fc1' must be a Linear\\(F, 128\\), got 96 -> 64", dict(fc1=nn.Linear(96, 64))),
            ("'fc1' must be a Linear", dict(fc1=nn.Conv2d(3, 3, 1))),
            ("'leaky' must be a LeakyReLU", dict(leaky=nn.ReLU())),
            ("slope of 'leaky'", dict(leaky=nn.LeakyReLU(1.5))),
            ("slope of 'leaky'", dict(leaky=nn.LeakyReLU(float("nan")))),
            ("'swarm' must be a Linear\\(128, O\\) or have such a 'layer_hypos'", dict(swarm=nn.Linear(64, 40))),
            ("'swarm' must be a Linear\\(128, O\\) or have such a 'layer_hypos'", dict(swarm=nn.ReLU())),
            ("HeadSpec", dict(swarm=nn.Linear(128, 41))),
            ("HeadSpec", dict(swarm=nn.Linear(128, 514)))]:
        with pytest.raises(ValueError, match="(fold_head: .*)?" + match):
            fold_head(**dict(good, **over))
    ok = hr.random_head(16, 4, 7, 40, 1)
    assert isinstance(check_head(ok), HeadSpec) and check_head(ok).w1.flags.c_contiguous
    for bad in (ok._replace(w1=np.zeros((64, 96))), ok._replace(c1=np.zeros(4)), ok._replace(w2=np.zeros((40, 64))), ok._replace(c2=np.zeros(41)),
                ok._replace(w2=np.zeros((41, 128)), c2=np.zeros(41)), ok._replace(w2=np.zeros((0, 128)), c2=np.zeros(0)),
                ok._replace(w2=np.zeros((514, 128)), c2=np.zeros(514)), ok._replace(slope=float("inf")), ok._replace(slope=-1.5),
                ok._replace(w1=np.zeros(96))):
        with pytest.raises(ValueError, match="HeadSpec"):
            check_head(bad)
    assert head_features(128, 10, 11) == 3200 and head_features(8, 3, 3) == 8


# ---- 3. the struct, the symbol and the kernel: no device needed ----------------------------------------------------------------------------------
def test_head_entry_point_refuses_null_arguments():
    lib = nm.load_library()
    assert "nmpc_mmp_head_f32" in nm.EXPORTED_SYMBOLS and hasattr(lib, "nmpc_mmp_head_f32")
    a = _capi.NmpcMmpHeadArgs()
    assert lib.nmpc_mmp_head_f32(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_head_f32(None, None) == -1


def test_head_args_layout_matches_the_c_compiler():
    fields = [f[0] for f in _capi.NmpcMmpHeadArgs._fields_]
    assert fields == ["M", "C", "H", "W", "O", "x", "w1", "c1", "w2", "c2", "slope", "out"]
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        body = "".join(f'printf(" %zu", offsetof(nmpc_mmp_head_args, {f}));' for f in fields)
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "nmpc_hip.h"\nint main(void){printf("%zu", sizeof(nmpc_mmp_head_args));'
                             + body + 'printf(" %d", NMPC_ABI_VERSION);return 0;}\n')
        exe = os.path.join(td, "sz")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert ctypes.sizeof(_capi.NmpcMmpHeadArgs) == out[0] == 80 and out[-1] == 5
    assert [getattr(_capi.NmpcMmpHeadArgs, f).offset for f in fields] == out[1:-1]


def test_head_kernel_uses_no_scratch_and_its_row_group_is_the_constant():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    nm.build_library()
    res = {kernel_resources.short_name(k): v for k, v in kernel_resources.kernel_resources(nm.library_path()).items()}
    mine = {k: v for k, v in res.items() if re.search(r"mmp_head_kernel", k)}
    assert len(mine) == 1, sorted(mine)
    header = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_mmp_head.h")).read()
    assert f"kHeadRows = {_capi.MMP_HEAD_ROWS};" in header and hr.ROWS == _capi.MMP_HEAD_ROWS == 16 and "kHeadFeatures = 128" in header
    for name, r in mine.items():
        print(name, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["lds_static"] == 4 * 128 * 16 * 4 + 512 * 17 * 4, (name, r)


# ---- 4. the controls of the bound, before any device run ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", hr.CASES, ids=hr.case_id)
def test_the_bound_admits_float32_and_refuses_the_wrong_variants(c):
    """On every case of the GPU tests: torch's own float32 head meets the bound (at most 0.023 of it), each wrong variant that
    differs from the definition on the plane at all misses it: "ceil" needs an odd side, "order" more than one pooled pixel; "sum"
    and "slope" apply everywhere. The smallest factors, all on the warehouse plane with two outputs, where 3 200 terms make the
    bound largest: "ceil" 9, "order" 48, "sum" 84, "slope" 34."""
    C, H, W, O = c
    x, spec, want, bound = hr.case("random", *c)
    assert want.shape == (hr.M_MAX, O) and (bound > 0).all() and hr.M_MAX == 2 * hr.ROWS + 1
    r32 = (np.abs(hr.torch_float32(x, spec) - want) / bound).max()
    line = f"{hr.case_id(c)}: torch float32 {r32:.4f}"
    assert r32 <= 1.0, "the bound refuses torch's own float32 head"
    applied = [w for w in WRONG if hr.applies(w, C, H, W)]
    assert set(applied) >= {"sum", "slope"} and ("ceil" in applied) == (H % 2 == 1 or W % 2 == 1) and ("order" in applied) == ((H // 2) * (W // 2) > 1)
    for wrong in WRONG:
        bad, _ = hr.head(x, spec, wrong=wrong)
        factor = (np.abs(bad - want) / bound).max()
        if wrong in applied:
            line += f", {wrong} x {factor:.0f}"
            assert factor > 1.0, f"the bound admits the wrong variant {wrong!r}"
        else:
            assert np.array_equal(bad, want)                   # (the variant is the definition on this plane)
    print(line)
    xi, si, wi, _ = hr.case("integer", *c)
    assert hr.integer_units(xi, si) < 2.0 ** 24
    assert np.array_equal(wi.astype(np.float32).astype(np.float64), wi) and np.array_equal(hr.torch_float32(xi, si), wi.astype(np.float32))


def test_the_cases():
    assert hr.PLANES == ((8, 2, 2), (8, 3, 3), (16, 4, 7), (128, 10, 11)) and hr.OUTPUTS == (2, 40, 512) and hr.ROWS_M == (1, 3, 2 * hr.ROWS + 1)
    assert any(hr.applies("ceil", *p) for p in hr.PLANES) and any(hr.applies("order", *p) for p in hr.PLANES)
