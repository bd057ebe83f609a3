"""Host test of the Winograd F(4x4,3x3) weight packer (csrc/conv3x3_winof4.hip): the matrices the library uses reproduce a 3x3 pad-1
convolution in float64, and the packed layout is the documented one.  No GPU: the packer and the matrices are host code of libpnpx.so."""
import ctypes as C

import numpy as np

from tfpnp_amd import _lib


def _matrices():
    g, bt, at = np.zeros((6, 3)), np.zeros((6, 6)), np.zeros((4, 6))
    _lib.lib().pnpx_winof4_matrices(g.ctypes.data, bt.ctypes.data, at.ctypes.data)
    return g, bt, at


def _conv3x3(x, w):
    """x [C][H][W], w [K][C][3][3] -> [K][H][W], zero padding 1, float64"""
    Cc, H, W = x.shape
    xp = np.zeros((Cc, H + 2, W + 2))
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((w.shape[0], H, W))
    for dy in range(3):
        for dx in range(3):
            out += np.einsum("kc,chw->khw", w[:, :, dy, dx], xp[:, dy:dy + H, dx:dx + W])
    return out


def test_library_matrices_reproduce_a_convolution():
    g, bt, at = _matrices()
    rng = np.random.default_rng(5)
    K, Cc, H, W = 4, 8, 8, 12
    w = rng.standard_normal((K, Cc, 3, 3))
    x = rng.standard_normal((Cc, H, W))
    u = np.einsum("ia,kcab,jb->kcij", g, w, g)                       # G g G^T
    xp = np.zeros((Cc, H + 2, W + 2))
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((K, H, W))
    for ty in range(H // 4):
        for tx in range(W // 4):
            d = xp[:, 4 * ty:4 * ty + 6, 4 * tx:4 * tx + 6]
            v = np.einsum("ia,cab,jb->cij", bt, d, bt)               # B^T d B
            m = np.einsum("kcij,cij->kij", u, v)
            out[:, 4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4] = np.einsum("pi,kij,qj->kpq", at, m, at)      # A^T M A
    ref = _conv3x3(x, w)
    assert np.abs(out - ref).max() / np.abs(ref).max() < 1e-12


def test_packed_layout_and_single_rounding():
    g, _, _ = _matrices()
    rng = np.random.default_rng(6)
    cout, cin = 128, 24
    w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
    dst = np.full(36 * cout * cin, np.nan, np.float32)
    assert _lib.lib().pnpx_winof4_pack(w.ctypes.data, cout, cin, dst.ctypes.data) == 0
    assert np.isfinite(dst).all()                                    # every slot written
    u = np.einsum("ia,kcab,jb->kcij", g, w.astype(np.float64), g)   # [cout][cin][6][6] in double, rounded once below
    # [cout/64][cin/8][stage 3][row 2][column pair 3][cout block 4][channel group 4][cout 16][k-step 2][column 2]
    p = dst.reshape(cout // 64, cin // 8, 3, 2, 3, 4, 4, 16, 2, 2)
    u10 = u.reshape(cout // 64, 4, 16, cin // 8, 4, 2, 3, 2, 3, 2)   # [ct][mb][m][ch][kq][ks][stage][row][pair][col]
    want = u10.transpose(0, 3, 6, 7, 8, 1, 4, 2, 5, 9)
    np.testing.assert_allclose(p, want.astype(np.float32), rtol=1.2e-7, atol=1e-30)
    # shapes the packer does not take
    assert _lib.lib().pnpx_winof4_pack(w.ctypes.data, 96, cin, dst.ctypes.data) != 0
    assert _lib.lib().pnpx_winof4_pack(w.ctypes.data, cout, 12, dst.ctypes.data) != 0
