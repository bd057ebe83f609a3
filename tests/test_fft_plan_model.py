"""CPU checks of tests/fft_plan_model.py: its constants are the ones in the source text of csrc/fft.hip and csrc/fft_lds.h,
and the case table of tests/test_gpu_operator_paths.py reaches every dispatch branch of the FFT launch plan at least once --
a later change to the plan (or to the table) cannot silently un-cover a branch."""
import os
import re

from tests import fft_plan_model as M
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "tfpnp_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _constexpr_int(text, name):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, f"constexpr int {name} not found"
    return int(eval(m.group(1), {"__builtins__": {}}))       # "1024" or "16 * 16 * 17"


def test_model_constants_are_the_sources():
    lds, fft = _src("fft_lds.h"), _src("fft.hip")
    assert _constexpr_int(lds, "FFT_TILE_POINTS") == M.FFT_TILE_POINTS == 1024
    assert _constexpr_int(lds, "FFT256_LINES") == M.FFT256_LINES == 16
    assert _constexpr_int(lds, "FFT_MAX_N") == M.FFT_MAX_N == 2048
    assert _constexpr_int(lds, "FFT_THREADS") == 256
    assert 8 * _constexpr_int(lds, "FFT256_LDS_F2") == M.FFT256_LDS_BYTES
    assert _constexpr_int(lds, "FFT_LDS_FLOOR") == M.FFT_LDS_FLOOR == 64 * 1024
    # the column clamp and the affine gate are literals of make_fft_plan
    body = fft[fft.index("int make_fft_plan("):fft.index("int fft2(")]
    clamp = re.findall(r"if\s*\(lc\s*>\s*(\d+)\)\s*lc\s*=\s*(\d+);", body)
    assert clamp == [(str(M.FFT_COL_CLAMP),) * 2], clamp
    gates = re.findall(r"opt_fft_affine\s*&&\s*n_img\s*>=\s*(\d+)", body)
    assert gates and set(gates) == {str(M.FFT_AFFINE_MIN_IMG)}, gates
    assert re.search(r"const int group = %d \* per_img;" % M.FFT_AFFINE_MIN_IMG, lds)          # xcd_affine_decode deals in eights
    # the tile geometry and the fast-path predicates, as the model restates them
    for needle in ("int lr = tile_points / W;", "if (lr > total_rows) lr = total_rows;", "int lc = tile_points / H;",
                   "if (lc > W) lc = W;", "if (lr > max_lr) lr = max_lr;", "if (lc > max_lc) lc = max_lc;",
                   "ctx->lds_block_limit / (sizeof(float2) * 2 * (size_t)(W + 1))",
                   "ctx->lds_block_limit / (sizeof(float2) * 2 * (size_t)(H + 1))", "P->rows.affine = (H % lr == 0) ? 1 : 0;",
                   "P->fast256_rows = (W == 256 && H % FFT256_LINES == 0);",
                   "P->fast256_cols = (H == 256 && W % FFT256_LINES == 0);",
                   "sizeof(float2) * 2 * (size_t)lr * (W + 1)", "sizeof(float2) * 2 * (size_t)lc * (H + 1)"):
        assert needle in body, needle
    assert "while (n % 4 == 0)" in fft and "for (int p = 2; p <= n; ++p)" in fft               # factorise: 4s, then primes


def test_model_reproduces_the_documented_plans():
    p = M.plan(9, 48, 256)
    assert (p.rows, p.cols, p.rows_affine, p.cols_affine, p.partial_group, p.partial_last_col_tile) == \
        ("fast256", "any[4,4,3]", True, True, True, True) and p.lc == 21
    p = M.plan(9, 256, 48)
    assert (p.rows, p.cols, p.lr, p.rows_affine, p.cols_affine) == ("any[4,4,3]", "fast256", 21, False, True)
    assert M.plan(3, 40, 256).rows == "pow2" and not M.plan(3, 40, 256).rows_affine and M.plan(8, 40, 256).rows_affine
    p = M.plan(10, 50, 39)
    assert (p.rows, p.cols, p.rows_affine, p.cols_affine) == ("any[3,13]", "any[2,5,5]", False, True)
    p = M.plan(9, 15, 33)
    assert p.odd_w and p.odd_h and p.row_tile_spans_images and p.lr == 31
    assert M.plan(12, 8, 16).lr == 64 and M.plan(12, 8, 16).row_tile_spans_images                 # 8 images per row tile
    p = M.plan(9, 4, 200)
    assert p.lc == 64 and 200 % 64 == 8 and p.partial_last_col_tile
    assert M.plan(1, 3, 1458).rows == "any[2,3,3,3,3,3,3]" and M.plan(1, 4, 1021).lr == 1
    assert M.plan(1, 1, 1).rows == "any[]" and M.plan(8, 1, 2).rows == "pow2"
    assert M.plan(1, 2048, 2048).lds_rows == 16 * 2049                                              # one line (+ ping-pong copy)
    asks = lambda s, t, lim: max(M.plan(*s, tile=t, lds_limit=lim).lds_rows, M.plan(*s, tile=t, lds_limit=lim).lds_cols)
    assert [asks(s, t, 0) for s, t in M.FFT_OVERSIZE_LEGS] == [66048, 132096, 163840]            # what the tile would ask for
    assert [asks(s, t, 64 * 1024) for s, t in M.FFT_OVERSIZE_LEGS] == [16 * 31 * 129, 16 * 31 * 129, 16 * 819 * 5]   # clamped
    assert [asks(s, t, 160 * 1024) for s, t in M.FFT_OVERSIZE_LEGS] == [66048, 132096, 163840]
    # the default tile is never clamped: at most one 2048-point line or 1024 points of short lines
    assert all(M.plan(*c) == M.plan(*c, lds_limit=0) for c in M.FFT_CASES)
    assert max(16 * max(1024 // n, 1) * (n + 1) for n in range(1, M.FFT_MAX_N + 1)) <= 32784 < M.FFT_LDS_FLOOR
    assert M.plan(11, 256, 256, fast=0).rows == "pow2" and not M.plan(11, 256, 256, affine=0).cols_affine


REQUIRED = (
    [("rows", k) for k in ("fast256", "pow2", "any")] + [("cols", k) for k in ("fast256", "pow2", "any")] +
    [("kinds", k) for k in (("fast256", "fast256"), ("fast256", "any"), ("any", "fast256"), ("pow2", "pow2"), ("any", "any"),
                            ("pow2", "any"), ("any", "pow2"))] +
    [(k, v) for k in ("rows_affine", "cols_affine", "partial_group", "row_tile_spans_images", "partial_last_col_tile", "odd_w",
                      "odd_h", "col_tile_clamped", "generic_256_point_line", "max_length") for v in (True, False)] +
    [("rows_affine,cols_affine", v) for v in ((False, False), (False, True), (True, True))] +
    [("radix", r) for r in (2, 3, 4, 5, 11, 13, 17)] +             # 17: a prime above 13 (127, 251, 509, 1021)
    [("rows.stages", n) for n in (0, 1, 2, 3, 7)] + [("cols.stages", n) for n in (0, 1, 2, 3)])


def _witnesses():
    seen = {}
    for case in M.FFT_CASES:
        for lab in M.labels(M.plan(*case)):
            seen.setdefault(lab, []).append(case)
    return seen


def test_case_table_reaches_every_branch():
    seen = _witnesses()
    missing = [lab for lab in REQUIRED if lab not in seen]
    assert not missing, f"no case of FFT_CASES reaches {missing}"
    # affine passes with full groups only and with a trailing partial group, on the fast and on the generic kernels
    both = {(M.plan(*c).rows == "fast256", M.plan(*c).partial_group) for c in M.FFT_CASES if M.plan(*c).rows_affine}
    assert both == {(True, True), (True, False), (False, True), (False, False)}, both
    sole = sorted({cs[0] for lab, cs in seen.items() if lab in REQUIRED and len(cs) == 1})
    print("sole witnesses:", sole)


def test_option_legs_reach_a_generic_pass_and_stay_in_the_option_range():
    """The tile size only matters on a generic pass: every option shape but the all-fast one has one, and the tile sweep moves
    its geometry; the over-size legs are exactly the ones above 64 KiB, the others stay below."""
    for s in M.FFT_OPTION_SHAPES:
        geoms = {(M.plan(*s, tile=t).lr, M.plan(*s, tile=t).lc) for t in M.FFT_TILES}
        p = M.plan(*s)
        if (p.rows, p.cols) == ("fast256", "fast256"):
            assert len(geoms) == 1
        else:
            assert len(geoms) >= 3, (s, geoms)
        assert s in M.FFT_CASES and M.plan(*s).partial_group
    assert max(M.FFT_TILES) == 8192                  # the documented range of option fft_tile (include/pnpx.h, api.hip)
    api = _src("api.hip")
    assert re.search(r'\{"fft_tile",\s*&pnpx_ctx::opt_fft_tile,\s*0,\s*8192\}', api)       # its row of the option table: name, field, min, max
    for s, t in M.FFT_OVERSIZE_LEGS:
        p = M.plan(*s, tile=t, lds_limit=0)
        assert p.rows != "fast256" and p.cols != "fast256" and max(p.lds_rows, p.lds_cols) > 64 * 1024
        p = M.plan(*s, tile=t)
        assert max(p.lds_rows, p.lds_cols) <= 64 * 1024
