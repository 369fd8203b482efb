// Stand-alone host program around csrc/triangulate_math.h: runs the per-track arithmetic of the triangulation kernels on the
// CPU, so that tests/test_host_triangulation.py can compare it with the restatement without a GPU and under the address
// and undefined-behaviour sanitizers.  Every track is run twice: serially (what one lane of the short-track kernel does) and
// as the long-track kernel does it — 64 per-lane triangles over the observations lane, lane + 64, ..., merged pairwise in
// the kernel's order.
//
// Input (text, from the file named on the command line): rank_tol optimize use_lost safe lost_sigma distance_threshold
// outlier_threshold noise_kind p0 .. p4 / n_cameras / per camera: kind has_sensor 17 doubles [12 doubles] / n_tracks / per
// track: m then m x (camera u v).  Output: per track two lines "status x y z iterations trials".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gtsam_petercdev_amd/csrc/triangulate_math.h"

using namespace gsx::trim;

static int wave_track(const Camera* cams, const int32_t* oc, const double* oz, int m, const Params& P, double* pt, int* cnt) {
  pt[0] = pt[1] = pt[2] = NAN;
  double T[64][10];
  int st[64];
  for (int lane = 0; lane < 64; ++lane) {
    tri_zero(T[lane]);
    st[lane] = ST_VALID;
    for (int i = lane; i < m; i += 64) {
      const int s = accumulate_observation(cams, oc, oz, m, i, P, T[lane]);
      st[lane] = s > st[lane] ? s : st[lane];
    }
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int lane = 0; lane < off; ++lane) {
      tri_merge(T[lane], T[lane + off]);
      st[lane] = st[lane + off] > st[lane] ? st[lane + off] : st[lane];
    }
  int status = st[0];
  if (status == ST_VALID) status = linear_finish(T[0], P, pt);
  return finish_track(cams, oc, oz, m, P, status, pt, cnt);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  Params P;
  int ok = fscanf(f, "%lf %d %d %d %lf %lf %lf %d %lf %lf %lf %lf %lf", &P.rank_tol, &P.optimize, &P.use_lost, &P.safe,
                  &P.lost_sigma, &P.landmark_distance_threshold, &P.outlier_threshold, &P.noise.kind, &P.noise.p[0],
                  &P.noise.p[1], &P.noise.p[2], &P.noise.p[3], &P.noise.p[4]);
  if (ok != 13) return 3;
  int n_cameras = 0;
  if (fscanf(f, "%d", &n_cameras) != 1 || n_cameras < 0) return 3;
  std::vector<Camera> cams((size_t)n_cameras);
  for (int c = 0; c < n_cameras; ++c) {
    int kind = 0, has_sensor = 0;
    double in[kCameraInDoubles], sensor[12];
    if (fscanf(f, "%d %d", &kind, &has_sensor) != 2) return 3;
    for (double& v : in)
      if (fscanf(f, "%lf", &v) != 1) return 3;
    if (has_sensor)
      for (double& v : sensor)
        if (fscanf(f, "%lf", &v) != 1) return 3;
    prepare_camera(kind, in, has_sensor ? sensor : nullptr, cams[(size_t)c]);
  }
  int n_tracks = 0;
  if (fscanf(f, "%d", &n_tracks) != 1 || n_tracks < 0) return 3;
  for (int t = 0; t < n_tracks; ++t) {
    int m = 0;
    if (fscanf(f, "%d", &m) != 1 || m < 0) return 3;
    std::vector<int32_t> oc((size_t)m);
    std::vector<double> oz(2 * (size_t)m);
    for (int i = 0; i < m; ++i) {
      if (fscanf(f, "%d %lf %lf", &oc[(size_t)i], &oz[2 * (size_t)i], &oz[2 * (size_t)i + 1]) != 3) return 3;
      if (oc[(size_t)i] < 0 || oc[(size_t)i] >= n_cameras) return 3;
    }
    double pt[3];
    int cnt[2];
    int st = triangulate_track(cams.data(), oc.data(), oz.data(), m, P, pt, cnt);
    printf("%d %.17g %.17g %.17g %d %d\n", st, pt[0], pt[1], pt[2], cnt[0], cnt[1]);
    st = m < 2 ? triangulate_track(cams.data(), oc.data(), oz.data(), m, P, pt, cnt)
               : wave_track(cams.data(), oc.data(), oz.data(), m, P, pt, cnt);
    printf("%d %.17g %.17g %.17g %d %d\n", st, pt[0], pt[1], pt[2], cnt[0], cnt[1]);
  }
  fclose(f);
  return 0;
}
