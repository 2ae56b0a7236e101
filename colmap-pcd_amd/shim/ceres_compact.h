// ceres_compact.h -- host half of the compact Ceres route (pcd_ba_evaluate_blocks_compact, include/pcdhip.h).
//
// The device ships one record {r0, r1, M row-major 2x3} per reprojection block, M = d r / d P with P = R(q) X + t.
// The three Jacobian blocks of the reference's functors (base/cost_functions.h:100-135, :319-355) are M times a factor
// that depends on the evaluation point alone, and Ceres hands that point to CostFunction::Evaluate:
//   jac_t = M       jac_X = M * D(q)       jac_q = M * dPdq(q, X)
// D = dP/dX and dPdq = dP/dq are those of csrc/ba_math.h reproj_eval: the derivative of Ceres'
// UnitQuaternionRotatePoint polynomial X + 2w (v x X) + 2 v x (v x X) w.r.t. X and all four quaternion components, q
// taken as it is (NOT normalised).  They are restated here in the same operation order, and the products are formed
// in the order of reproj_jacobians, so that -- compiled without FMA contraction (-ffp-contract=off), as the device code
// is -- the rebuilt rows are the rows pcd_ba_evaluate_blocks returns, bit for bit.
// Plain C++, no HIP, header-only.
#pragma once

namespace colmap_hip {

// q = (w, x, y, z), X the world point, rec = {r0, r1, M00, M01, M02, M10, M11, M12}.
// jac_q [2][4], jac_t [2][3], jac_X [2][3] row-major; any of them may be NULL (not written).
inline void ExpandReprojectionBlock(const double q[4], const double X[3], const double rec[8], double* jac_q,
                                    double* jac_t, double* jac_X) {
  const double* M = rec + 2;
  const double w = q[0], a = q[1], bq = q[2], c = q[3];
  if (jac_t)
    for (int k = 0; k < 6; ++k) jac_t[k] = M[k];
  if (jac_X) {
    // D = I + 2w[v]x + 2(v v^T - |v|^2 I)
    double D[9];
    D[0] = 1.0 - 2.0 * (bq * bq + c * c); D[1] = 2.0 * (a * bq - w * c);       D[2] = 2.0 * (a * c + w * bq);
    D[3] = 2.0 * (a * bq + w * c);        D[4] = 1.0 - 2.0 * (a * a + c * c);  D[5] = 2.0 * (bq * c - w * a);
    D[6] = 2.0 * (a * c - w * bq);        D[7] = 2.0 * (bq * c + w * a);       D[8] = 1.0 - 2.0 * (a * a + bq * bq);
    for (int r = 0; r < 2; ++r)
      for (int k = 0; k < 3; ++k)
        jac_X[3 * r + k] = M[3 * r] * D[k] + M[3 * r + 1] * D[3 + k] + M[3 * r + 2] * D[6 + k];
  }
  if (jac_q) {
    // dP/dw = 2 v x X ; dP/dv_k = 2w (e_k x X) + 2 e_k (v.X) + 2 v X_k - 4 X v_k
    double dPdq[12];
    const double cx = bq * X[2] - c * X[1], cy = c * X[0] - a * X[2], cz = a * X[1] - bq * X[0];
    dPdq[0] = 2.0 * cx; dPdq[4] = 2.0 * cy; dPdq[8] = 2.0 * cz;
    const double vX = a * X[0] + bq * X[1] + c * X[2];
    const double vq[3] = {a, bq, c};
    // e_0 x X = (0, -X2, X1); e_1 x X = (X2, 0, -X0); e_2 x X = (-X1, X0, 0)
    const double eX[3][3] = {{0.0, -X[2], X[1]}, {X[2], 0.0, -X[0]}, {-X[1], X[0], 0.0}};
    for (int k = 0; k < 3; ++k)
      for (int i = 0; i < 3; ++i)
        dPdq[4 * i + 1 + k] = 2.0 * w * eX[k][i] + (i == k ? 2.0 * vX : 0.0) + 2.0 * vq[i] * X[k] - 4.0 * X[i] * vq[k];
    for (int r = 0; r < 2; ++r)
      for (int k = 0; k < 4; ++k)
        jac_q[4 * r + k] = M[3 * r] * dPdq[k] + M[3 * r + 1] * dPdq[4 + k] + M[3 * r + 2] * dPdq[8 + k];
  }
}

}  // namespace colmap_hip
