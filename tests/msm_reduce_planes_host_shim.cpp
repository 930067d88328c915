// The plane arithmetic of the bucket reduction's tail (zecale_amd/csrc/msm_plan.hpp: tail_*) behind a C interface for
// tests/test_msm_reduce_planes_host.py: plain g++, no HIP.
#include "../zecale_amd/csrc/msm_plan.hpp"

using namespace zkhip::plan;
typedef unsigned long long u64;

extern "C" {
int t_lo_bits(int c) { return lo_bits(c); }
int t_hi_bits(int c) { return hi_bits(c); }
int t_fan_in_const() { return TAIL_FAN_IN; }
int t_weight_planes(u64 N) { return tail_weight_planes(N); }
int t_planes(u64 N, int total) { return tail_planes(N, total != 0); }
int t_fan_in(u64 left) { return tail_fan_in(left); }
int t_levels(u64 N) { return tail_levels(N); }
u64 t_level_outputs(int planes, int G, u64 N, int level) { return tail_level_outputs(planes, G, N, level); }
u64 t_cap_tail(int W, u64 N, int which) { return cap_tail(W, N, which); }
u64 t_cap_hilo(int W, int c) { return cap_hilo(W, c); }
}
