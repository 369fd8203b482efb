// schedule_options.cpp — the one reader of the schedule switches (gsx_internal.h: ScheduleOptions; product, host only).
#include <algorithm>
#include <cstdlib>

#include "gsx_internal.h"

namespace gsx {

ScheduleOptions schedule_options_from_env() {
  ScheduleOptions o;
  auto set = [](const char* name) { return std::getenv(name) != nullptr; };
  auto not_zero = [](const char* name) {   // the pack switches: "=0" means off
    const char* e = std::getenv(name);
    return !(e && std::atoi(e) == 0);
  };
  if (const char* e = std::getenv("GSX_TREE_TIERS")) {
    o.tree_bounds.clear();
    o.tree_threads.clear();
    int v[2] = {0, 0}, k = 0;
    bool any = false;
    for (const char* q = e;; ++q) {
      if (*q >= '0' && *q <= '9') {
        v[k] = v[k] * 10 + (*q - '0');
        any = true;
      } else if (*q == ':') {
        k = 1;
      } else {
        if (any && v[0] > 0) {
          o.tree_bounds.push_back(std::min(v[0], kSmallMaxN));
          o.tree_threads.push_back(std::max(0, std::min(512, (v[1] + 63) / 64 * 64)));   // (the kernel's launch bound)
        }
        v[0] = v[1] = k = 0;
        any = false;
        if (!*q) break;
      }
    }
  }
  o.medium = set("GSX_MEDIUM");
  o.side = !set("GSX_SIDE_OFF");
  if (const char* e = std::getenv("GSX_SIDE_MIN")) o.side_min = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("GSX_ND_LEAF")) o.nd_leaf = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("GSX_SMALL_THREADS_SHIFT")) o.small_threads_shift = std::atoi(e);
  o.h_tile = !set("GSX_H_TILE_OFF");
  o.fused_star = not_zero("GSX_FUSED_STAR");
  o.star_leaf_pack = not_zero("GSX_STAR_LEAF_PACK");
  o.bs_leaf_pack = not_zero("GSX_BS_LEAF_PACK");
  o.bs_tree = !set("GSX_BS_TREE_OFF");
  o.linerr_from_step = !set("GSX_LINERR_DIRECT");
  return o;
}

}  // namespace gsx
