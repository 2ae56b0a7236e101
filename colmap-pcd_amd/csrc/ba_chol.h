// ba_chol.h -- dense fp64 factor-and-solve on the device (ba_chol.hip): blocked right-looking Cholesky with the
// right-hand side carried as one more row of the matrix.  Knows nothing about bundle adjustment.  Internal.
#pragma once
#include <cstddef>

#include "common.h"

namespace pcd {

constexpr int kCholNB = 96;   // panel width: 16 pose slots; a multiple of the 16 x 16 matrix-pipe tile

// Scratch layout, row-major with leading dimension np = chol_padded(n): rows [0, np) hold the matrix (lower triangle;
// the upper one is never read), identity on the padding.  One more block of kCholNB rows follows: its row 0 is the
// right-hand side (after the factorisation y = L^-1 b), its row 1 receives x, the others stay 0 and only keep the
// row tiles whole.  A last block of kCholNB rows receives the factors of the diagonal blocks, L_kk in columns
// [96 k, 96 k + 96): a diagonal block of the matrix itself is read by every workgroup of its panel's launch and is
// therefore never written by that launch.
inline int chol_padded(int n) { return (n + kCholNB - 1) / kCholNB * kCholNB; }
inline size_t chol_scratch_doubles(int n) { return ((size_t)chol_padded(n) + 2 * kCholNB) * (size_t)chol_padded(n); }

// Zeroes what the solve reads (the tiles of the lower triangle and the right-hand side's block), puts the identity on
// the padding and resets the status record.  The caller then fills the lower triangle of rows [0, n) and the
// right-hand side row (chol_fill_dense, or a kernel of its own).
void chol_begin(double* A, int n, pcd_ba_chol_info* status, hipStream_t s);
// lower triangle of S [n][n] (row-major, caller memory, not modified) and rhs [n] into the scratch
void chol_fill_dense(double* A, int n, const double* S, const double* rhs, hipStream_t s);
// Factorisation and both triangular solves; x [n] (0 when the factorisation failed) and, if asked for, a copy of the
// status record.  Plain launches, no synchronisation.
void chol_factor_solve(double* A, int n, pcd_ba_chol_info* status, double* x, pcd_ba_chol_info* info_out, hipStream_t s);

}  // namespace pcd
