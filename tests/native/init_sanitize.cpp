// The host side of the Pose3 initializer (csrc/init_graph.cpp: pose graph, adjacency, the two internal descriptions) and the
// per-rotation arithmetic the device kernels run (csrc/init_math.h, compiled here for the host) under AddressSanitizer +
// UBSan: tests/test_host_initialize_pose3.py builds this with g++ -fsanitize=address,undefined and runs it on the golden
// g2o files.  No GPU, no HIP.
//   init_sanitize <golden dir>                 the lowering of every 3-D golden file; prints "<file> ok" per file
//   init_sanitize <golden dir> <matrices>      additionally Rot3::ClosestTo (initm::closest_rotation) of every 3 x 3 matrix
//                                              of the text file (9 numbers per line, row-major): "R <9 numbers>" per line
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../gtsam_petercdev_amd/csrc/gsx_internal.h"
#include "../../gtsam_petercdev_amd/csrc/init_math.h"

extern "C" {
gsx_status gsx_dataset_get(const gsx_dataset* d, gsx_problem_desc* desc, const double** values, int64_t* n_values);
}

static int check_file(const std::string& dir, const char* name) {
  gsx_dataset* ds = nullptr;
  if (gsx_read_g2o((dir + "/" + name).c_str(), 1, &ds) != GSX_OK) return 1;
  gsx_problem_desc desc;
  const double* values = nullptr;
  int64_t nv = 0;
  if (gsx_dataset_get(ds, &desc, &values, &nv) != GSX_OK) return 1;
  gsx::PoseGraph G;
  std::string err;
  if (gsx::build_pose_graph(&desc, G, err) != GSX_OK) {
    std::fprintf(stderr, "%s: build_pose_graph: %s\n", name, err.c_str());
    return 1;
  }
  if (!G.anchored || !G.all_touched || (int)G.adj.size() != 2 * (int)G.from.size()) return 1;
  // the two internal descriptions must be well-formed problems
  gsx::OwnedDesc R, P;
  std::vector<int> var_of_node, edges;
  gsx::lower_relaxed(&desc, G, R, var_of_node, edges);
  gsx::HostProblem HP;
  gsx_problem_desc view = R.view();
  if (gsx::lower_problem(&view, HP, err) != GSX_OK || HP.jac_size != 21 * (int64_t)edges.size() + 12) {
    std::fprintf(stderr, "%s: relaxed system: %s\n", name, err.c_str());
    return 1;
  }
  gsx::lower_anchor_graph(&desc, G, P, var_of_node);
  view = P.view();
  if (gsx::lower_problem(&view, HP, err) != GSX_OK || HP.n_vars != G.n_poses + 1) {
    std::fprintf(stderr, "%s: anchor graph: %s\n", name, err.c_str());
    return 1;
  }
  // the public structure query, sizes first
  int32_t ne = 0;
  if (gsx_pose3_init_structure(&desc, &ne, nullptr, nullptr, nullptr, nullptr, 0) != GSX_OK) return 1;
  std::vector<int32_t> ef(ne), et(ne), ap(G.n_poses + 2), adj(2 * (size_t)ne);
  if (gsx_pose3_init_structure(&desc, &ne, ef.data(), et.data(), ap.data(), adj.data(), (int64_t)adj.size()) != GSX_OK) return 1;
  if (gsx_pose3_init_structure(&desc, &ne, nullptr, nullptr, nullptr, adj.data(), (int64_t)adj.size() - 1) != GSX_E_INVALID)
    return 1;
  // one gradient evaluation per edge on the file's own values (Logmap / Expmap branches on real data)
  double acc = 0.0;
  for (int e = 0; e < ne; ++e) {
    double g[3], I[9];
    gsx::initm::mat_identity(I);
    gsx::initm::gradient_tron(I, &G.rot[9 * (size_t)e], 6.010534238540223, 1.0, g);
    acc += g[0] + g[1] + g[2];
  }
  if (!(acc == acc)) return 1;
  gsx_dataset_free(ds);
  std::printf("%s ok\n", name);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  for (const char* name : {"pose3example.txt", "pose3example-grid.txt", "simpleGraph10gradIter.txt", "sphere2500.txt"})
    if (check_file(dir, name)) return 1;
  // a malformed description: a factor that names a variable out of range
  {
    const uint64_t keys[2] = {1, 2};
    const int32_t types[2] = {GSX_VAR_POSE3, GSX_VAR_POSE3}, dims[2] = {6, 6};
    const int32_t f_type[1] = {GSX_F_BETWEEN}, f_rows[1] = {6}, key_ptr[2] = {0, 2}, f_vars[2] = {0, 7}, kinds[1] = {GSX_NOISE_UNIT};
    const int64_t meas_ptr[2] = {0, 12}, noise_ptr[2] = {0, 0};
    const double meas[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, noise[1] = {0};
    gsx_problem_desc d{2, keys, types, dims, 1, f_type, f_rows, key_ptr, f_vars, meas_ptr, meas, kinds, noise_ptr, noise};
    gsx::PoseGraph G;
    std::string err;
    if (gsx::build_pose_graph(&d, G, err) != GSX_E_INVALID) return 1;
  }
  if (argc > 2) {
    std::FILE* f = std::fopen(argv[2], "r");
    if (!f) return 2;
    double M[9], R[9];
    while (std::fscanf(f, "%lf %lf %lf %lf %lf %lf %lf %lf %lf", M, M + 1, M + 2, M + 3, M + 4, M + 5, M + 6, M + 7, M + 8) == 9) {
      gsx::initm::closest_rotation(M, R);
      std::printf("R %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7],
                  R[8]);
    }
    std::fclose(f);
  }
  return 0;
}
