"""A plain Python restatement of the FFT launch plan (csrc/fft.hip:make_fft_plan, csrc/fft_lds.h) and the case table of
tests/test_gpu_operator_paths.py.  TEST INFRASTRUCTURE: the model names the dispatch branches a shape takes, so that the
CPU test tests/test_fft_plan_model.py can assert that the GPU case table reaches every one of them, and that the
constants below are still the ones in the source text."""
from collections import namedtuple

# Mirrors of the source constants (tests/test_fft_plan_model.py reads them back out of fft.hip / fft_lds.h)
FFT_TILE_POINTS = 1024     # fft_lds.h: complex points per workgroup tile when option fft_tile is 0
FFT256_LINES = 16          # fft_lds.h: lines per tile of the register-radix-16 kernels
FFT_COL_CLAMP = 64         # fft.hip: `if (lc > 64) lc = 64`
FFT_AFFINE_MIN_IMG = 8     # fft.hip: `n_img >= 8` gate of the XCD-affine mapping (images are dealt in groups of 8)
FFT_MAX_N = 2048           # fft_lds.h: longest line
FFT256_LDS_BYTES = 8 * 16 * 16 * 17     # fft_lds.h: FFT256_LDS_F2 float2 words, static
FFT_LDS_FLOOR = 64 * 1024  # fft_lds.h: the least per-block LDS limit make_fft_plan clamps its tiles to

Plan = namedtuple("Plan", "rows cols rows_affine cols_affine partial_group row_tile_spans_images partial_last_col_tile "
                          "odd_w odd_h lds_rows lds_cols lr lc n_img H W")


def radices(N):
    """fft.hip:factorise -- 4s first, then the prime factors in ascending order."""
    out, n = [], N
    while n % 4 == 0:
        out.append(4)
        n //= 4
    p = 2
    while p <= n:
        while n % p == 0:
            out.append(p)
            n //= p
        p += 1
    return out


def _pass_kind(N, fast256):
    if fast256:
        return "fast256"
    if N >= 2 and N & (N - 1) == 0:          # fft_lds.h:ilog2_exact (length 1 is NOT a power of two there: zero stages)
        return "pow2"
    return "any[" + ",".join(map(str, radices(N))) + "]"


def plan(n_img, H, W, tile=0, affine=1, fast=1, lds_limit=FFT_LDS_FLOOR):
    """The branch labels of make_fft_plan(n_img, H, W) under options fft_tile / fft_affine / fft_fast on a device whose per-block LDS
    limit is `lds_limit` bytes (0: no clamp -- what the tile would ask for)."""
    assert 1 <= H <= FFT_MAX_N and 1 <= W <= FFT_MAX_N and n_img > 0
    total_rows = n_img * H
    tile_points = tile if tile > 0 else FFT_TILE_POINTS
    lr = min(max(tile_points // W, 1), total_rows)
    lc = min(max(tile_points // H, 1), W, FFT_COL_CLAMP)
    if lds_limit:
        lds_limit = max(lds_limit, FFT_LDS_FLOOR)
        lr, lc = min(lr, lds_limit // (16 * (W + 1))), min(lc, lds_limit // (16 * (H + 1)))
    gate = bool(affine) and n_img >= FFT_AFFINE_MIN_IMG
    rows_affine = gate and H % lr == 0
    cols_affine = gate
    fast_rows = bool(fast) and W == 256 and H % FFT256_LINES == 0
    fast_cols = bool(fast) and H == 256 and W % FFT256_LINES == 0
    if gate and fast_rows:
        rows_affine = True
    return Plan(rows=_pass_kind(W, fast_rows), cols=_pass_kind(H, fast_cols),
                rows_affine=bool(rows_affine), cols_affine=bool(cols_affine),
                partial_group=bool((rows_affine or cols_affine) and n_img % 8 != 0),
                row_tile_spans_images=bool(not fast_rows and lr > H),
                partial_last_col_tile=bool(not fast_cols and W % lc != 0),
                odd_w=bool(W & 1), odd_h=bool(H & 1),
                lds_rows=FFT256_LDS_BYTES if fast_rows else 16 * lr * (W + 1),
                lds_cols=FFT256_LDS_BYTES if fast_cols else 16 * lc * (H + 1),
                lr=FFT256_LINES if fast_rows else lr, lc=FFT256_LINES if fast_cols else lc, n_img=n_img, H=H, W=W)


# (n_img, H, W) of test_gpu_operator_paths.py::test_fft2_case_matrix_vs_fp64 and what each one pins
FFT_CASES = [
    (16, 256, 256),    # both passes fast, affine, full groups only
    (11, 256, 256),    # both fast, affine, with a trailing partial group
    (7, 256, 256),     # both fast, no affine
    (9, 48, 256),      # fast rows, generic cols any[4,4,3], affine, partial last column tile
    (9, 256, 48),      # generic rows (lr = 21, rows.affine = 0), fast cols (affine)
    (3, 40, 256),      # generic 256-point rows, H % 16 != 0
    (8, 40, 256),      # the same with rows.affine = 1
    (19, 128, 128),    # generic pow2, both affine, partial group
    (17, 96, 80),      # mixed radix, both affine
    (10, 50, 39),      # rows.affine = 0 with cols.affine = 1
    (9, 15, 33),       # odd centered lengths with n_img >= 8, row tile spans images
    (12, 8, 16),       # row tile spans 8 images
    (9, 4, 200),       # column tile clamped to 64, last tile 8 columns
    (2, 127, 251),     # prime lengths
    (1, 509, 16),      # prime length
    (1, 4, 1021),      # prime length, one thread per line
    (1, 3, 1458),      # seven stages
    (1, 2048, 2048),   # maximum size, per value
    (8, 1, 2),         # degenerate lengths
    (1, 2, 1),
    (1, 1, 1),
]

# shapes of the option legs (fft_affine x fft_tile bit-identity; fft_fast = 0 on those with a 256-point line)
FFT_OPTION_SHAPES = [(9, 48, 256), (10, 50, 39), (19, 128, 128), (11, 256, 256)]
FFT_TILES = (0, 512, 2048, 4096, 8192)
FFT_GENERIC256_SHAPES = [(9, 48, 256), (9, 256, 48), (11, 256, 256)]      # fft_fast = 0: their 256-point lines on the generic kernel
# generic shapes whose tile would ask for more than 64 KiB of dynamic LDS without the clamp: (shape, fft_tile)
FFT_OVERSIZE_LEGS = [((9, 128, 128), 4096), ((9, 128, 128), 8192), ((3, 2048, 4), 8192)]


def labels(p):
    """The set of (label, value) pairs a plan witnesses; radix lists count per radix, so that `any` is not one opaque value."""
    out = set()
    for axis, kind in (("rows", p.rows), ("cols", p.cols)):
        out.add((axis, kind.split("[")[0]))
        if kind.startswith("any["):
            rs = [int(r) for r in kind[4:-1].split(",") if r]
            out.add((axis + ".stages", min(len(rs), 7)))
            out.update(("radix", min(r, 17)) for r in rs)      # 17 stands for "a prime above 13" (the O(R^2) stage at large R)
    for k in ("rows_affine", "cols_affine", "partial_group", "row_tile_spans_images", "partial_last_col_tile", "odd_w", "odd_h"):
        out.add((k, getattr(p, k)))
    out.add(("rows_affine,cols_affine", (p.rows_affine, p.cols_affine)))
    out.add(("col_tile_clamped", p.cols != "fast256" and p.lc == FFT_COL_CLAMP))
    out.add(("kinds", (p.rows.split("[")[0], p.cols.split("[")[0])))
    out.add(("generic_256_point_line", (p.W == 256 and p.rows != "fast256") or (p.H == 256 and p.cols != "fast256")))
    out.add(("max_length", p.H == FFT_MAX_N or p.W == FFT_MAX_N))
    return out
