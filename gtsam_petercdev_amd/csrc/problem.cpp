// problem.cpp — validation and lowering of gsx_problem_desc into host tables.
#include <cmath>
#include <algorithm>

#include "gsx_internal.h"

namespace gsx {

static int state_dim(int type, int dim) {
  switch (type) {
    case GSX_VAR_VECTOR: return dim;
    case GSX_VAR_POSE2: return 3;
    case GSX_VAR_POSE3: return 12;
    case GSX_VAR_CAMERA: return 17;
    case GSX_VAR_ROT3: return 9;
    case GSX_VAR_UNIT3: return 3;
    case GSX_VAR_ESSENTIAL: return 12;
  }
  return -1;
}

gsx_status check_direction_states(const HostProblem& P, const double* values, std::string& err) {
  for (int v : P.direction_vars)
    if (!direction_state_ok(P.types[v], values + P.state_off[v])) {
      err = "variable " + std::to_string(v) + " (key " + std::to_string((unsigned long long)P.keys[v]) + "), a " +
            direction_type_name(P.types[v]) + ": its direction is not of unit length";
      return GSX_E_INVALID;
    }
  return GSX_OK;
}

gsx_status lower_problem(const gsx_problem_desc* d, HostProblem& P, std::string& err) {
  if (!d || d->n_vars < 0 || d->n_factors < 0) {
    err = "null or negative-sized description";
    return GSX_E_INVALID;
  }
  P.n_vars = d->n_vars;
  P.n_factors = d->n_factors;
  P.con_factor.clear();
  P.con_row.clear();
  P.con_mu.clear();
  P.direction_vars.clear();
  P.keys.assign(d->var_keys, d->var_keys + d->n_vars);
  P.types.assign(d->var_types, d->var_types + d->n_vars);
  P.dims.assign(d->var_dims, d->var_dims + d->n_vars);
  P.state_off.resize(P.n_vars + 1);
  P.tan_off.resize(P.n_vars + 1);
  P.state_size = P.tan_size = 0;
  for (int v = 0; v < P.n_vars; ++v) {
    if (v > 0 && !(P.keys[v] > P.keys[v - 1])) {
      err = "var_keys must be strictly ascending";
      return GSX_E_INVALID;
    }
    const int t = P.types[v];
    const int expect[7] = {P.dims[v], 3, 6, 9, 3, 2, 5};
    if (t < 0 || t > 6 || P.dims[v] != expect[t] || P.dims[v] <= 0 || (t == GSX_VAR_VECTOR && P.dims[v] > 64)) {
      err = "bad variable type/dim at variable " + std::to_string(v);
      return GSX_E_INVALID;
    }
    P.state_off[v] = (int)P.state_size;
    P.tan_off[v] = (int)P.tan_size;
    if (is_direction_type(t)) P.direction_vars.push_back(v);
    P.state_size += state_dim(t, P.dims[v]);
    P.tan_size += P.dims[v];
  }
  P.state_off[P.n_vars] = (int)P.state_size;
  P.tan_off[P.n_vars] = (int)P.tan_size;
  const int nf = P.n_factors;
  P.f_type.assign(d->f_type, d->f_type + nf);
  P.f_rows.assign(d->f_rows, d->f_rows + nf);
  P.f_key_ptr.assign(d->f_key_ptr, d->f_key_ptr + nf + 1);
  P.f_vars.assign(d->f_vars, d->f_vars + (nf ? d->f_key_ptr[nf] : 0));
  P.f_meas_ptr.assign(d->f_meas_ptr, d->f_meas_ptr + nf + 1);
  P.meas.assign(d->meas, d->meas + (nf ? d->f_meas_ptr[nf] : 0));
  P.f_noise_kind.assign(d->f_noise_kind, d->f_noise_kind + nf);
  P.f_noise_ptr.assign(d->f_noise_ptr, d->f_noise_ptr + nf + 1);
  P.noise.assign(d->noise, d->noise + (nf ? d->f_noise_ptr[nf] : 0));
  P.f_jac_off.resize(nf + 1);
  P.f_cols.resize(nf);
  P.jac_size = 0;
  bool any_attitude = false;
  for (int f = 0; f < nf; ++f) {
    const int nk = P.f_key_ptr[f + 1] - P.f_key_ptr[f];
    const int m = P.f_rows[f];
    int cols = 1;
    for (int k = P.f_key_ptr[f]; k < P.f_key_ptr[f + 1]; ++k) {
      const int v = P.f_vars[k];
      if (v < 0 || v >= P.n_vars) {
        err = "factor " + std::to_string(f) + " refers to a variable out of range";
        return GSX_E_INVALID;
      }
      for (int k2 = P.f_key_ptr[f]; k2 < k; ++k2)
        if (P.f_vars[k2] == v) {
          err = "factor " + std::to_string(f) + " lists a variable twice";
          return GSX_E_INVALID;
        }
      cols += P.dims[v];
    }
    const int64_t nmeas = P.f_meas_ptr[f + 1] - P.f_meas_ptr[f];
    const int64_t nnoise = P.f_noise_ptr[f + 1] - P.f_noise_ptr[f];
    bool ok = m > 0 && m <= 64;
    auto tv = [&](int slot) { return P.types[P.f_vars[P.f_key_ptr[f] + slot]]; };
    auto dv = [&](int slot) { return P.dims[P.f_vars[P.f_key_ptr[f] + slot]]; };
    switch (P.f_type[f]) {
      case GSX_F_LINEAR:
        ok = ok && nk >= 1 && nk <= 8 && nmeas == (int64_t)m * cols;
        break;
      case GSX_F_PRIOR:
        ok = ok && nk == 1 && m == dv(0) && nmeas == state_dim(tv(0), dv(0)) && m <= 9;
        if (ok && is_direction_type(tv(0)) && !direction_state_ok(tv(0), P.meas.data() + P.f_meas_ptr[f])) {
          err = "factor " + std::to_string(f) + ": the direction of the prior on a " + direction_type_name(tv(0)) +
                " is not of unit length";
          return GSX_E_INVALID;
        }
        break;
      case GSX_F_BETWEEN:
        for (int k = 0; k < nk && k < 2; ++k)  // neither type is a group
          if (is_direction_type(tv(k))) {
            err = "factor " + std::to_string(f) + ": GSX_F_BETWEEN on variable " + std::to_string(P.f_vars[P.f_key_ptr[f] + k]) +
                  ", a " + direction_type_name(tv(k)) + " (not a group)";
            return GSX_E_INVALID;
          }
        ok = ok && nk == 2 && tv(0) == tv(1) && dv(0) == dv(1) && tv(0) != GSX_VAR_CAMERA && m == dv(0) &&
             nmeas == state_dim(tv(0), dv(0)) && m <= 9;
        break;
      case GSX_F_SFM:
        ok = ok && nk == 2 && tv(0) == GSX_VAR_CAMERA && tv(1) == GSX_VAR_VECTOR && dv(1) == 3 && m == 2 && nmeas == 2;
        break;
      case GSX_F_BEARINGRANGE:
        ok = ok && nk == 2 && tv(0) == GSX_VAR_POSE2 && tv(1) == GSX_VAR_VECTOR && dv(1) == 2 && m == 2 && nmeas == 2;
        break;
      case GSX_F_PROJECTION:  // 7, or 7 + 12 with body_P_sensor
        ok = ok && nk == 2 && tv(0) == GSX_VAR_POSE3 && tv(1) == GSX_VAR_VECTOR && dv(1) == 3 && m == 2 &&
             (nmeas == 7 || nmeas == 7 + 12);
        break;
      case GSX_F_RANGE:  // (POSE2 | POSE3) to a point of its space or to a pose of its kind; + the first key's state
                         // layout with body_T_sensor
        ok = ok && nk == 2 && (tv(0) == GSX_VAR_POSE2 || tv(0) == GSX_VAR_POSE3) &&
             (tv(1) == tv(0) || (tv(1) == GSX_VAR_VECTOR && dv(1) == (tv(0) == GSX_VAR_POSE2 ? 2 : 3))) && m == 1 &&
             (nmeas == 1 || nmeas == 1 + state_dim(tv(0), dv(0)));
        break;
      case GSX_F_BEARING:
        ok = ok && nk == 2 && tv(0) == GSX_VAR_POSE2 && tv(1) == GSX_VAR_VECTOR && dv(1) == 2 && m == 1 && nmeas == 1;
        break;
      case GSX_F_STEREO:
        ok = ok && nk == 2 && tv(0) == GSX_VAR_POSE3 && tv(1) == GSX_VAR_VECTOR && dv(1) == 3 && m == 3 &&
             (nmeas == 9 || nmeas == 9 + 12);
        break;
      case GSX_F_SFM2:
        ok = ok && nk == 3 && tv(0) == GSX_VAR_POSE3 && tv(1) == GSX_VAR_VECTOR && dv(1) == 3 && tv(2) == GSX_VAR_VECTOR &&
             dv(2) == 5 && m == 2 && nmeas == 2;
        break;
      case GSX_F_SMART_PROJECTION: {  // 2 .. 8 POSE3 keys; 11 doubles, optionally body_P_sensor (12), then 2 nk pixels
        ok = ok && nk >= 2 && nk <= 8 && m == 2 * nk - 3 && (nmeas == 11 + 2 * nk || nmeas == 11 + 12 + 2 * nk);
        for (int k = 0; ok && k < nk; ++k) {
          if (tv(k) == GSX_VAR_ROT3) {
            err = "factor " + std::to_string(f) + ": GSX_F_SMART_PROJECTION on variable " +
                  std::to_string(P.f_vars[P.f_key_ptr[f] + k]) + ", a GSX_VAR_ROT3 (its keys are POSE3)";
            return GSX_E_INVALID;
          }
          ok = tv(k) == GSX_VAR_POSE3;
        }
        // SmartFactorBase "needs isotropic"; only ZERO_ON_DEGENERACY (1) of the degeneracy modes
        const int nkind = P.f_noise_kind[f];
        ok = ok && (nkind == GSX_NOISE_UNIT || nkind == GSX_NOISE_ISOTROPIC);
        if (ok && P.meas[P.f_meas_ptr[f] + 10] != 1.0) {
          err = "factor " + std::to_string(f) + ": only ZERO_ON_DEGENERACY is taken by GSX_F_SMART_PROJECTION";
          return GSX_E_INVALID;
        }
        break;
      }
      case GSX_F_TRANSLATION:
        ok = ok && nk == 2 && tv(0) == GSX_VAR_VECTOR && dv(0) == 3 && tv(1) == GSX_VAR_VECTOR && dv(1) == 3 && m == 3 &&
             nmeas == 3;
        break;
      case GSX_F_BILINEAR_TRANSLATION:
        ok = ok && nk == 3 && tv(0) == GSX_VAR_VECTOR && dv(0) == 3 && tv(1) == GSX_VAR_VECTOR && dv(1) == 3 &&
             tv(2) == GSX_VAR_VECTOR && dv(2) == 1 && m == 3 && nmeas == 3;
        break;
      case GSX_F_GPS:  // (POSE3): nT, or nT and bL; (POSE3, VECTOR(3)): nT, the lever arm a variable
        ok = ok && nk >= 1 && m == 3 && tv(0) == GSX_VAR_POSE3 &&
             ((nk == 1 && (nmeas == 3 || nmeas == 6)) || (nk == 2 && tv(1) == GSX_VAR_VECTOR && dv(1) == 3 && nmeas == 3));
        break;
      case GSX_F_POSE_TRANSLATION_PRIOR:
        ok = ok && nk == 1 && ((tv(0) == GSX_VAR_POSE2 && m == 2) || (tv(0) == GSX_VAR_POSE3 && m == 3)) && nmeas == m;
        break;
      case GSX_F_POSE_ROTATION_PRIOR:
        ok = ok && nk == 1 && ((tv(0) == GSX_VAR_POSE2 && m == 1 && nmeas == 1) || (tv(0) == GSX_VAR_POSE3 && m == 3 && nmeas == 9));
        break;
      case GSX_F_ATTITUDE:
        ok = ok && nk == 1 && (tv(0) == GSX_VAR_ROT3 || tv(0) == GSX_VAR_POSE3) && m == 2 && nmeas == 6;
        for (int q = 0; ok && q < 2; ++q) {
          const double* u = P.meas.data() + P.f_meas_ptr[f] + 3 * q;
          if (!(std::fabs(std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) - 1.0) <= 1e-9)) {
            err = "factor " + std::to_string(f) + ": " + (q ? "bMeasured" : "nRef") + " of GSX_F_ATTITUDE is not of unit length";
            return GSX_E_INVALID;
          }
        }
        any_attitude = any_attitude || ok;
        break;
      case GSX_F_MAG:
        ok = ok && nk == 1 &&
             (((tv(0) == GSX_VAR_ROT3 || tv(0) == GSX_VAR_POSE3) && m == 3) || (tv(0) == GSX_VAR_POSE2 && m == 2)) &&
             nmeas == 3 * m;
        break;
      case GSX_F_ESSENTIAL:  // vA, vB
        ok = ok && nk == 1 && tv(0) == GSX_VAR_ESSENTIAL && m == 1 && nmeas == 6;
        break;
      case GSX_F_ESSENTIAL_DEPTH:  // dP1, pn, f; with cRb behind them EssentialMatrixFactor3
        ok = ok && nk == 2 && tv(0) == GSX_VAR_ESSENTIAL && tv(1) == GSX_VAR_VECTOR && dv(1) == 1 && m == 2 &&
             (nmeas == 6 || nmeas == 15);
        break;
      case GSX_F_ESSENTIAL_CALIB:  // pA, pB
        ok = ok && nk == 2 && tv(0) == GSX_VAR_ESSENTIAL && tv(1) == GSX_VAR_VECTOR && dv(1) == 5 && m == 1 && nmeas == 4;
        break;
      case GSX_F_ESSENTIAL_CONSTRAINT:  // the measured E: R, direction
        ok = ok && nk == 2 && tv(0) == GSX_VAR_POSE3 && tv(1) == GSX_VAR_POSE3 && m == 5 && nmeas == 12;
        if (ok && !direction_state_ok(GSX_VAR_ESSENTIAL, P.meas.data() + P.f_meas_ptr[f])) {
          err = "factor " + std::to_string(f) + ": the direction of the measured E of GSX_F_ESSENTIAL_CONSTRAINT is not of unit length";
          return GSX_E_INVALID;
        }
        break;
      default:
        ok = false;
    }
    {
      const int kind = P.f_noise_kind[f], loss = kind >> 4;
      const int64_t extra = loss ? 1 : 0;  // a robust model appends its k / c
      ok = ok && kind >= 0 && loss <= 3;
      if (loss && P.f_type[f] == GSX_F_LINEAR) ok = false;  // a given linear factor is already whitened
      switch (kind & GSX_NOISE_BASE_MASK) {
        case GSX_NOISE_UNIT: ok = ok && nnoise == 0 + extra; break;
        case GSX_NOISE_ISOTROPIC: ok = ok && nnoise == 1 + extra; break;
        case GSX_NOISE_DIAGONAL: ok = ok && nnoise == m + extra; break;
        case GSX_NOISE_GAUSSIAN: ok = ok && nnoise == (int64_t)m * m + extra; break;
        case GSX_NOISE_CONSTRAINED: ok = ok && nnoise == 2 * (int64_t)m && !loss; break;
        default: ok = false;
      }
      if (loss && ok) ok = P.noise[P.f_noise_ptr[f + 1] - 1] > 0;
      const int base = kind & GSX_NOISE_BASE_MASK;
      if (ok && (base == GSX_NOISE_ISOTROPIC || base == GSX_NOISE_DIAGONAL || base == GSX_NOISE_CONSTRAINED)) {
        const int64_t ns = base == GSX_NOISE_ISOTROPIC ? 1 : m;
        for (int64_t k = 0; k < ns; ++k) {
          const double sg = P.noise[P.f_noise_ptr[f] + k];
          // a sigma of exactly 0 in a diagonal model is a hard-constraint row (noiseModel::Constrained, NoiseModel.h:389-500)
          const bool constraint = sg == 0.0 && base != GSX_NOISE_ISOTROPIC && !loss;
          if (!constraint && (!(sg > 0) || !std::isfinite(sg))) {
            err = "factor " + std::to_string(f) + ": sigma " + std::to_string(sg) +
                  " (a hard constraint is a sigma of exactly 0 in a GSX_NOISE_DIAGONAL / GSX_NOISE_CONSTRAINED model)";
            return GSX_E_INVALID;
          }
          if (constraint) {
            const double mu = base == GSX_NOISE_CONSTRAINED ? P.noise[P.f_noise_ptr[f] + m + k] : 1000.0;
            if (!(mu > 0) || !std::isfinite(mu)) {
              err = "factor " + std::to_string(f) + ": constraint weight mu " + std::to_string(mu);
              return GSX_E_INVALID;
            }
            P.con_factor.push_back(f);
            P.con_row.push_back((int)k);
            P.con_mu.push_back(mu);
          }
        }
      }
    }
    if (!ok) {
      err = "malformed factor " + std::to_string(f);
      return GSX_E_INVALID;
    }
    P.f_cols[f] = cols;
    P.f_jac_off[f] = P.jac_size;
    P.jac_size += (int64_t)m * cols;
  }
  P.f_jac_off[nf] = P.jac_size;
  // GSX_F_ATTITUDE: B = nRef.basis() (3 x 2 row-major) behind the two directions, computed here once per factor
  if (any_attitude) {
    std::vector<double> meas;
    std::vector<int64_t> ptr(nf + 1, 0);
    for (int f = 0; f < nf; ++f) {
      ptr[f] = (int64_t)meas.size();
      meas.insert(meas.end(), P.meas.begin() + P.f_meas_ptr[f], P.meas.begin() + P.f_meas_ptr[f + 1]);
      if (P.f_type[f] == GSX_F_ATTITUDE) {
        double B[6];
        unit3_basis(P.meas.data() + P.f_meas_ptr[f], B);
        meas.insert(meas.end(), B, B + 6);
      }
    }
    ptr[nf] = (int64_t)meas.size();
    P.meas.swap(meas);
    P.f_meas_ptr.swap(ptr);
  }
  // Hard-constraint rows on the device: a DIAGONAL model whose constraint rows carry sigma = 1 / sqrt(mu).  Every kernel
  // then treats them as ordinary rows — the graph error gets mu e^2 / 2 for a violated constraint
  // (Constrained::squaredMahalanobisDistance, NoiseModel.cpp:438-444), the linearized error likewise
  // (JacobianFactor::error with the unit() model, JacobianFactor.cpp:508-513), and J'J a penalty term that is constant on
  // the feasible set — and the factorization eliminates the rows EXACTLY by constraint pivots (solver.hip: dev_factorize launches the constraint_* kernels of constraint.hip).
  if (!P.con_factor.empty() || std::find(P.f_noise_kind.begin(), P.f_noise_kind.end(), (int)GSX_NOISE_CONSTRAINED) !=
                                   P.f_noise_kind.end()) {
    std::vector<double> noise;
    std::vector<int64_t> ptr(nf + 1, 0);
    size_t ci = 0;
    for (int f = 0; f < nf; ++f) {
      const int base = P.f_noise_kind[f] & GSX_NOISE_BASE_MASK, m = P.f_rows[f];
      const int64_t b = P.f_noise_ptr[f], e = P.f_noise_ptr[f + 1];
      ptr[f] = (int64_t)noise.size();
      if (base == GSX_NOISE_DIAGONAL || base == GSX_NOISE_CONSTRAINED) {
        for (int k = 0; k < m; ++k) {
          double sg = P.noise[b + k];
          if (ci < P.con_factor.size() && P.con_factor[ci] == f && P.con_row[ci] == k) sg = 1.0 / std::sqrt(P.con_mu[ci++]);
          noise.push_back(sg);
        }
        if (base == GSX_NOISE_DIAGONAL)
          for (int64_t k = b + m; k < e; ++k) noise.push_back(P.noise[k]);   // (a robust model's parameter)
        else
          P.f_noise_kind[f] = GSX_NOISE_DIAGONAL;
      } else {
        noise.insert(noise.end(), P.noise.begin() + b, P.noise.begin() + e);
      }
    }
    ptr[nf] = (int64_t)noise.size();
    P.noise.swap(noise);
    P.f_noise_ptr.swap(ptr);
  }
  return GSX_OK;
}

}  // namespace gsx
