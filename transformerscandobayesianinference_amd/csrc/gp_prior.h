// What gp_prior.hip offers other files: its blocked Cholesky on a matrix the caller has filled (the hyper-parameter fit, gp_fit.hip) and the switch of
// PFN_TUNE_GP_PLANES (pfn_set_tuning, pfn_api.hip).
#pragma once
#include "pfn_host.h"

namespace pfn {

struct GpArgs {
  float* x;        // [B,S,nf] uniform(0,1) features: generated when seed_x != 0, else taken as input
  const float* z;  // [B,S] base normals: taken as input when non-null, else generated
  float* y;        // [B,S] output sample
  float* K;        // [B,S,S] workspace (f32)
  const float* lengthscale;  // [B,nf] per dataset / per feature
  const float* outputscale;  // [B]
  const float* noise;        // [B]
  int B, S, nf, kernel;      // kernel: 0 RBF, 1 Matern-5/2
  unsigned long long seed, offset;
  int gen_x, gen_z;
  int* info;                 // [B] 0 ok, else index+1 of the first non-positive pivot
  // posterior mode (pfn_gp_posterior): the same factorisation run as a forward solve  w = L^-1 y_data  -- y holds the
  // running residual (y_data on entry), w the solution, and every panel subtracts L[rows, panel] w[panel] from the
  // residual below it where the sampler adds L[rows, panel] z[panel] to the draw
  float* w;                  // [B,S]; null = sampler mode
  // scratch behind K (gp_workspace_bytes): the two scaled fp16 planes (hi, lo) of the current outer block's solved panel, written by gp_trsm_wide_kernel and
  // read by gp_syrk_planes_kernel -- [B][2 planes][16 k-chunks][plane_rows][16] fp16.  null = the trailing update splits the f32 panel itself (gp_syrk_kernel)
  void* planes;
  long plane_rows;           // rows allocated per slab (>= S - 256, a multiple of 128)
};
int64_t gp_workspace_bytes(int B, int S);      // K [B,S,S] f32 + the plane scratch
void gp_attach_planes(GpArgs& a);               // points a.planes behind a.K (a workspace of gp_workspace_bytes)
int launch_gp_factor(const GpArgs& a, hipStream_t s);      // the blocked Cholesky (+ y = L z / w = L^-1 y) on an a.K that is already filled
void set_gp_planes(int on);                     // PFN_TUNE_GP_PLANES (see gp_check_workspace, gp_prior.hip)

}  // namespace pfn
