// Stand-alone host program around csrc/smart_math.h: runs the per-factor arithmetic of the smart projection kernels on the
// CPU, so that tests/test_host_smart_factor.py can judge it like the device — without a GPU and under the address and
// undefined-behaviour sanitizers.  Every factor is evaluated through a sequence of pose sets with ONE cache, as a handle
// does; every linearization is done twice: serially (E and its reflectors once, then column after column) and in the
// column-per-lane order of smart_linearize_kernel (every column rebuilds E and its reflectors for itself).
//
// Input (text, from the file named on the command line): n_factors / per factor: nk nmeas sigma, nmeas doubles (the meas
// layout of include/gsx.h), n_steps, per step: kind (0 linearize, 1 error) then nk x 12 pose doubles.
// Output per step: "status retriangulated x y z error", then for a linearize step two lines (serial, lanes) of the
// m x (6 nk + 1) block, column-major ("zero" flag first: 1 when the block is the all-zero one).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gtsam_petercdev_amd/csrc/smart_math.h"

using namespace gsx;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int n_factors = 0;
  if (fscanf(f, "%d", &n_factors) != 1 || n_factors < 0) return 3;
  for (int q = 0; q < n_factors; ++q) {
    int nk = 0, nmeas = 0, n_steps = 0;
    double sigma = 1.0;
    if (fscanf(f, "%d %d %lf", &nk, &nmeas, &sigma) != 3) return 3;
    if (nk < 2 || nk > smart::kMaxViews || (nmeas != smart::kHead + 2 * nk && nmeas != smart::kHead + 12 + 2 * nk)) return 3;
    std::vector<double> meas((size_t)nmeas);
    for (double& v : meas)
      if (fscanf(f, "%lf", &v) != 1) return 3;
    const double* sensor = smart::sensor_of(meas.data(), nmeas, nk);
    const double* z = smart::pixels_of(meas.data(), nmeas, nk);
    const double inv_sigma = 1.0 / sigma;
    trim::Params prm;
    smart::triangulation_params(meas.data(), prm);
    std::vector<double> cache(12 * (size_t)nk, 0.0);
    int status = smart::kNever;
    double point[3] = {NAN, NAN, NAN};
    if (fscanf(f, "%d", &n_steps) != 1 || n_steps < 0) return 3;
    for (int s = 0; s < n_steps; ++s) {
      int kind = 0;
      if (fscanf(f, "%d", &kind) != 1) return 3;
      std::vector<double> poses(12 * (size_t)nk);
      for (double& v : poses)
        if (fscanf(f, "%lf", &v) != 1) return 3;
      std::vector<trim::Camera> cams((size_t)nk);
      for (int i = 0; i < nk; ++i) smart::view_camera(poses.data() + 12 * i, meas.data(), sensor, cams[(size_t)i]);
      const bool retri =
          smart::decide_retriangulate(cams.data(), nk, meas[smart::M_RETRIANGULATION], status, cache.data());
      if (retri) status = smart::triangulate(cams.data(), z, nk, prm, point);
      bool ok = status == trim::ST_VALID;
      double err = 0.0;
      if (ok) err = smart::reprojection_error(cams.data(), z, nk, point, inv_sigma, &ok);
      printf("%d %d %.17g %.17g %.17g %.17g\n", status, (int)retri, point[0], point[1], point[2], err);
      if (kind != 0) continue;
      const int m = 2 * nk - 3, ncols = 6 * nk + 1;
      for (int order = 0; order < 2; ++order) {
        std::vector<double> block((size_t)m * ncols, 0.0);
        bool valid = status == trim::ST_VALID;
        if (valid && order == 0) {   // serial: one E, one set of reflectors
          double E[3 * smart::kMaxRows], beta[3], x[smart::kMaxRows];
          valid = smart::build_column(cams.data(), sensor, z, nk, point, inv_sigma, 0, E, x);
          if (valid) {
            smart::reflectors(E, 2 * nk, beta);
            for (int c = 0; c < ncols; ++c) {
              double E2[3 * smart::kMaxRows];
              smart::build_column(cams.data(), sensor, z, nk, point, inv_sigma, c, E2, x);
              smart::apply_reflectors(E, beta, 2 * nk, x);
              for (int r = 0; r < m; ++r) block[(size_t)c * m + r] = x[r + 3];
            }
          }
        } else if (valid) {          // as the lanes of a wave: every column on its own
          for (int c = 0; c < ncols && valid; ++c) {
            double x[smart::kMaxRows];
            valid = smart::block_column(cams.data(), sensor, z, nk, point, inv_sigma, c, x);
            for (int r = 0; valid && r < m; ++r) block[(size_t)c * m + r] = x[r + 3];
          }
          if (!valid) block.assign(block.size(), 0.0);
        }
        printf("%d", valid ? 0 : 1);
        for (double v : block) printf(" %.17g", v);
        printf("\n");
      }
    }
  }
  fclose(f);
  return 0;
}
