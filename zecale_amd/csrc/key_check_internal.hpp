// What key_check.hip shares with phase2.hip: the point checks of one element of a key (device and host), the pair relation and the
// random-combination sums.  Defined in key_check.hip; not visible outside the library.
#pragma once
#include <vector>

#include "api_internal.hpp"
#include "device_buffer.hpp"

namespace zkhip {

struct KeyCheckCounters {
  unsigned long long infinity, refused[3], points;
  uint32_t first;       // min over the refused points of (index in the element << 2) | (code - ZKHIP_VERIFY_ENCODING)
  uint32_t pad;
};

#pragma GCC visibility push(hidden)
namespace keycheck {

struct Element { const uint64_t* p; size_t n; bool g2; };

// the device side of the point checks: a stream, the staging buffer of one chunk and the counters of one element
struct KeyCheckDev {
  DeviceStream st;
  DeviceBuffer<uint64_t> d_pts, d_r;
  DeviceBuffer<uint8_t> d_codes;
  DeviceBuffer<KeyCheckCounters> d_cnt;
  std::vector<hipEvent_t> ev;
  ~KeyCheckDev() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};

double now_ms();
bool is_infinity(const uint64_t* p);
size_t chunk_hook();       // zkhip_internal_key_check_set_chunk's value (0: the rule of key_check_chunk)
int dev_open(KeyCheckDev& w);      // the stream, the counters and r's words
void host_check_element(const Element& el, zkhip_key_element_report* rep);
int dev_check_element(KeyCheckDev& w, const Element& el, size_t chunk, zkhip_key_element_report* rep, double* longest_ms);
bool same_multiple(const uint64_t* p1, const uint64_t* p2);
void host_combination(const uint64_t* pts, const uint64_t* rho, size_t n, uint64_t out[24]);
int dev_combination(const uint64_t* pts, const std::vector<uint64_t>& scalars, size_t n, uint64_t out[24]);

}  // namespace keycheck
#pragma GCC visibility pop

}  // namespace zkhip
