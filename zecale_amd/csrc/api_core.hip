// C ABI (include/zkhip.h): the library's state, device selection, errors, raw device / host memory, host field and point helpers.
#include <string.h>

#include "api_internal.hpp"

using namespace zkhip::api;

namespace zkhip {
namespace api {
Lib g;

int fail(int code, const char* msg) {
  snprintf(t_err, sizeof t_err, "%s", msg);
  return code;
}
// a failed call of the MSM engine: the context holds its message
int ctx_fail(int code, const MsmCtx* cx) { return fail(code, cx->errbuf); }
int cur_dev() { return t_dev >= 0 ? t_dev : g.default_device; }
// bind the calling thread to device d (it must have been initialised)
int bind_dev(int d) {
  if (d < 0 || d >= ZK_MAX_DEVICES || !g.dev[d].inited) return fail(ZKHIP_ERR_STATE, "zkhip_init not called (for this device)");
  hipError_t e = hipSetDevice(d);
  if (e != hipSuccess) { snprintf(t_err, sizeof t_err, "hipSetDevice(%d): %s", d, hipGetErrorString(e)); return ZKHIP_ERR_HIP; }
  return ZKHIP_OK;
}
}  // namespace api
}  // namespace zkhip

extern "C" {

int zkhip_init(int device) {
  std::lock_guard<std::mutex> lk(g.mu);
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) return fail(ZKHIP_ERR_NO_DEVICE, "no HIP device (the gfx950 kernels are the only compute path)");
  if (device < 0 || device >= count || device >= ZK_MAX_DEVICES) return fail(ZKHIP_ERR_ARG, "device index out of range");
  API_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  API_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    snprintf(t_err, sizeof t_err, "device %d is %s, this library contains gfx950 code only", device, prop.gcnArchName);
    return ZKHIP_ERR_NO_DEVICE;
  }
  g.dev[device].inited = true;
  if (g.default_device < 0) g.default_device = device;
  t_dev = device;
  return ZKHIP_OK;
}

int zkhip_set_device(int device) {
  int rc = bind_dev(device);
  if (rc == ZKHIP_OK) t_dev = device;
  return rc;
}
int zkhip_get_device(void) { return cur_dev(); }

void zkhip_shutdown(void) {
  std::lock_guard<std::mutex> lk(g.mu);
  for (int d = 0; d < ZK_MAX_DEVICES; d++) {
    if (!g.dev[d].inited) continue;
    std::lock_guard<std::mutex> lkd(g.dev[d].mu);
    if (hipSetDevice(d) == hipSuccess) g.dev[d].ps.release();
    g.dev[d].inited = false;
  }
  g.default_device = -1;
  t_dev = -1;
}

const char* zkhip_strerror(int code) {
  switch (code) {
    case ZKHIP_OK: return "ok";
    case ZKHIP_ERR_ARG: return "bad argument";
    case ZKHIP_ERR_NO_DEVICE: return "no gfx950 device";
    case ZKHIP_ERR_HIP: return "HIP runtime error";
    case ZKHIP_ERR_STATE: return "library not initialised";
    case ZKHIP_ERR_NO_TICKET: return "no such ticket";
    case ZKHIP_ERR_REFUSED: return "input refused by a checked prover";
    default: return "unknown error";
  }
}
const char* zkhip_last_error(void) { return t_err; }

// device memory for callers without a HIP runtime of their own (the *_dev entry points take such pointers)
int zkhip_device_alloc(size_t bytes, void** out) {
  BIND_CUR();
  if (!out) return fail(ZKHIP_ERR_ARG, "null pointer");
  API_HIP(hipMalloc(out, bytes ? bytes : 1));
  return ZKHIP_OK;
}
int zkhip_device_free(void* p) {
  if (p) API_HIP(hipFree(p));
  return ZKHIP_OK;
}
int zkhip_device_copy_in(void* dst, const void* src, size_t bytes) {
  BIND_CUR();
  if (bytes && (!dst || !src)) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (bytes) {
    API_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    API_HIP(hipStreamSynchronize(0));
  }
  return ZKHIP_OK;
}

int zkhip_device_copy_out(void* dst_host, const void* src_device, size_t bytes) {
  BIND_CUR();
  if (bytes && (!dst_host || !src_device)) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (bytes) API_HIP(hipMemcpy(dst_host, src_device, bytes, hipMemcpyDeviceToHost));
  return ZKHIP_OK;
}

int zkhip_device_memory(size_t* free_bytes, size_t* total_bytes) {
  BIND_CUR();
  size_t f = 0, t = 0;
  API_HIP(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return ZKHIP_OK;
}

int zkhip_device_count(void) {
  int count = 0;
  return hipGetDeviceCount(&count) == hipSuccess ? count : 0;
}

// uniform in [0, r): 377-bit draws from the OS, rejected when >= r (a value in [0, r) read as a Montgomery residue is a uniform
// field element either way)
int zkhip_fr_random(uint64_t out[6]) {
  if (!out) return fail(ZKHIP_ERR_ARG, "null pointer");
  FILE* f = fopen("/dev/urandom", "rb");
  if (!f) return fail(ZKHIP_ERR_STATE, "cannot open /dev/urandom");
  for (;;) {
    if (fread(out, 8, 6, f) != 6) { fclose(f); return fail(ZKHIP_ERR_STATE, "short read from /dev/urandom"); }
    out[5] &= ((uint64_t)1 << 57) - 1;               // r has 377 bits
    bool less = false;
    for (int i = 5; i >= 0; i--) {
      if (out[i] != FrParams::P64[i]) { less = out[i] < FrParams::P64[i]; break; }
    }
    if (less) break;
  }
  fclose(f);
  return ZKHIP_OK;
}

int zkhip_to_canonical(int which, const uint64_t* in, uint64_t* out) {
  using namespace host;
  if (!in || !out) return ZKHIP_ERR_ARG;
  if (which == 0) HFq::from_limbs(in).to_canonical(out);
  else if (which == 1) HFr::from_limbs(in).to_canonical(out);
  else return ZKHIP_ERR_ARG;
  return ZKHIP_OK;
}

int zkhip_jac_to_affine(const uint64_t jac[36], uint64_t aff[24]) {
  using namespace host;
  if (!jac || !aff) return ZKHIP_ERR_ARG;
  HJac p;
  p.X = HFq::from_limbs(jac); p.Y = HFq::from_limbs(jac + 12); p.Z = HFq::from_limbs(jac + 24);
  HFq x, y;
  p.to_affine(x, y);
  x.to_limbs(aff); y.to_limbs(aff + 12);
  return ZKHIP_OK;
}

int zkhip_jac_add(const uint64_t a[36], const uint64_t b[36], uint64_t out[36]) {
  using namespace host;
  if (!a || !b || !out) return ZKHIP_ERR_ARG;
  HJac p, q;
  p.X = HFq::from_limbs(a); p.Y = HFq::from_limbs(a + 12); p.Z = HFq::from_limbs(a + 24);
  q.X = HFq::from_limbs(b); q.Y = HFq::from_limbs(b + 12); q.Z = HFq::from_limbs(b + 24);
  HJac r = p.add(q);
  r.X.to_limbs(out); r.Y.to_limbs(out + 12); r.Z.to_limbs(out + 24);
  return ZKHIP_OK;
}

// pinned host memory for callers without a HIP runtime of their own (source of zkhip_msm_stream_submit_host's asynchronous copies)
int zkhip_host_alloc(size_t bytes, void** out) {
  BIND_CUR();
  if (!out) return fail(ZKHIP_ERR_ARG, "null pointer");
  API_HIP(hipHostMalloc(out, bytes ? bytes : 1));
  return ZKHIP_OK;
}
int zkhip_host_free(void* p) {
  if (p) API_HIP(hipHostFree(p));
  return ZKHIP_OK;
}

// (multi_device.cpp: a worker thread's failure text travels to the thread that called the library)
void zkhip_internal_set_error(const char* msg) { snprintf(t_err, sizeof t_err, "%s", msg ? msg : ""); }

}  // extern "C"
