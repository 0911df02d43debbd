// Process-wide knobs (include/tzrec_hip.h: tzr_tune).  Every knob is an int defined beside the launcher that reads it;
// defaults are chosen there.
#include <string.h>

#include "tzr_common.h"

extern int g_tzr_fwd_tile_b;
extern int g_tzr_fwd_variant;
extern int g_tzr_fwd_plan;
extern int g_tzr_bwd_ch;
extern int g_tzr_bwd_force_prep;
extern int g_tzr_bwd_one_wg_heavy;
extern int g_tzr_bwd_no_fuse_sort;
extern int g_tzr_bwd_direct;
extern int g_tzr_bwd_direct_ch;
extern int g_tzr_bwd_direct_hot;
extern int g_tzr_bwd_direct_debug;
extern int g_tzr_ia_bwd_wgs;
extern int g_tzr_ia_fwd_wgs;
extern int g_tzr_ia_gen_wgs;
extern int g_tzr_it_wgs;
extern int g_tzr_it_fwd_stagger;
extern int g_tzr_wg_debug;
extern int g_tzr_mlp_mfma;
extern int g_tzr_linear_bwd_wg;
extern int g_tzr_gemm_rows_wg;

static const struct {
  const char* name;
  int* value;
} kKnobs[] = {
    {"fwd_tile_b", &g_tzr_fwd_tile_b},
    {"fwd_variant", &g_tzr_fwd_variant},
    {"fwd_plan", &g_tzr_fwd_plan},
    {"bwd_ch", &g_tzr_bwd_ch},
    {"bwd_force_prep", &g_tzr_bwd_force_prep},
    {"bwd_one_wg_heavy", &g_tzr_bwd_one_wg_heavy},
    {"bwd_no_fuse_sort", &g_tzr_bwd_no_fuse_sort},
    {"bwd_direct", &g_tzr_bwd_direct},
    {"bwd_direct_ch", &g_tzr_bwd_direct_ch},
    {"bwd_direct_hot", &g_tzr_bwd_direct_hot},
    {"bwd_direct_debug", &g_tzr_bwd_direct_debug},
    {"ia_bwd_wgs", &g_tzr_ia_bwd_wgs},
    {"ia_fwd_wgs", &g_tzr_ia_fwd_wgs},
    {"ia_gen_wgs", &g_tzr_ia_gen_wgs},
    {"it_wgs", &g_tzr_it_wgs},
    {"it_fwd_stagger", &g_tzr_it_fwd_stagger},
    {"wg_debug", &g_tzr_wg_debug},
    {"mlp_mfma", &g_tzr_mlp_mfma},
    {"linear_bwd_wg", &g_tzr_linear_bwd_wg},
    {"gemm_rows_wg", &g_tzr_gemm_rows_wg},
};

extern "C" int tzr_tune(const char* name, int value) {
  if (!name) return TZR_ERR_INVALID;
  for (const auto& k : kKnobs)
    if (!strcmp(name, k.name)) {
      *k.value = value;
      return TZR_OK;
    }
  return TZR_ERR_INVALID;
}
