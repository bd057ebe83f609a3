// The 1-D matrices of Winograd F(4, 3) with the points (0, +-1, +-1/2, inf): y = A^T [(G g) * (B^T d)].  Rows of B^T are scaled to the
// product of the point differences and the rows of G by its inverse (tools/wino_f4_probe.py cook_toom with these points gives the same
// numbers).  conv3x3_winof4.hip: the packer computes G g G^T from WINOF4_G in double; the kernel's bt_row / at_rows spell out
// WINOF4_BT / WINOF4_AT.
#pragma once

namespace pnpx {

constexpr double WINOF4_G[6][3] = {{4.0, 0.0, 0.0},
                                   {2.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0},
                                   {2.0 / 3.0, -2.0 / 3.0, 2.0 / 3.0},
                                   {-8.0 / 3.0, -4.0 / 3.0, -2.0 / 3.0},
                                   {-8.0 / 3.0, 4.0 / 3.0, -2.0 / 3.0},
                                   {0.0, 0.0, 1.0}};
constexpr double WINOF4_BT[6][6] = {{0.25, 0.0, -1.25, 0.0, 1.0, 0.0},  {0.0, -0.25, -0.25, 1.0, 1.0, 0.0}, {0.0, 0.25, -0.25, -1.0, 1.0, 0.0},
                                    {0.0, -0.5, -1.0, 0.5, 1.0, 0.0},   {0.0, 0.5, -1.0, -0.5, 1.0, 0.0},   {0.0, 0.25, 0.0, -1.25, 0.0, 1.0}};
constexpr double WINOF4_AT[4][6] = {{1.0, 1.0, 1.0, 1.0, 1.0, 0.0},
                                    {0.0, 1.0, -1.0, 0.5, -0.5, 0.0},
                                    {0.0, 1.0, 1.0, 0.25, 0.25, 0.0},
                                    {0.0, 1.0, -1.0, 0.125, -0.125, 1.0}};

}  // namespace pnpx
