// Test hook zkhip_internal_point_ops_selftest (tests/test_point_ops_gpu.py; cases and exact expectations from
// tests/point_ops_cases.py): ONE point operation of ec.cuh, ec_mem.cuh or ec_edw.cuh per launch, on operands given limb by limb and
// staged in exactly the form the function takes in the library.  Nothing is converted, reduced or normalised on the way in or out.
// A translation unit of its own: no kernel of the library is compiled differently because this one exists.
//
// Lanes: 64 a workgroup.  Case i runs in lane i % 64 of wave i / 64; for the quad forms in lanes 4 (i % 16) .. 4 (i % 16) + 3 of
// wave i / 16, all four lanes with the same references.  The op switch is uniform (one kernel instance per op).
//
// in, per case (PO_ROW_IN words): A = X | Y | ZZ | ZZZ (X | Y | Z | T for the Edwards forms), 27 limbs each; B = the same, or the
// affine operand of the register forms (x | y, 27 limbs each), or the packed operand in its own words (AffPacked: 48, EdwPacked: 72);
// then neg, three entry words (index | neg << 31 into `table`) and the entry count of the lockstep run.
// out, per case (PO_ROW_OUT words): the four coordinates of the updated accumulator (an X that lives PACKED in LDS comes back as its 24
// packed words and three zeros; edw_from_affine: the 72 packed words), one flag word, then B as it stands after the op.  The flag is
// the function's return value; for a void function it is fp_is_zero_2p of the result's ZZ / Z (infinite / empty), taken from the
// copied-out words: nothing reads A after the op except the copy-out.
//
// Staging.  Register forms: Fq / XYZZ values.  Packed operands: AffPacked / EdwPacked in global memory.  Memory operands: an XyzzRef
// into an array the HOST laid out with plain index arithmetic - mem 0: limb-major, stride = the number of cases (make_ref); mem 1: the
// slot structure (make_slot_ref) - and reads back the same way, so mem_ld / mem_st are checked against an addressing that is not
// theirs.  LDS forms: lds_st_packed for X, lds_st for the two other images (ZK_LDS_STRIDE), Y in a register; their `acc` / `spill`
// reference points into the A array.  Every form that takes an XyzzRef runs with BOTH kinds of reference (the library hands its
// reduction kernels either through make_in_ref, and the accumulation's spill target is a slot); the forms that take none (the five
// register forms, edw_madd_lds_regy, edw_from_affine, the lockstep run) accept mem 0 only.
//
// The lockstep run is driven as k_accumulate_edw_lock (msm.hip) drives it: the wave's trip count is its first lane's count (the
// cases of a wave come in descending count), edw_pre_issue then edw_open_lds_pre for entry 0, edw_madd_lds_pre for the others, with
// the same has_e1 / has_e2 and the same hand-over of T0 .. T2 and e2.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "ec_edw.cuh"
#include "msm.h"

namespace zkhip {

enum PointOp : int {
  PO_DBL_AFFINE = 0, PO_DBL, PO_MADD, PO_ADD, PO_NEG,                                                   // ec.cuh, registers
  PO_MADD_MEM, PO_MADD_LDS_REGY, PO_ADD_LDS_REGY, PO_ADD_MEM_S, PO_DBL_MEM, PO_ADD_MEM_QUAD, PO_DBL_MEM_QUAD,   // ec_mem.cuh
  PO_EDW_MADD_LDS_REGY, PO_EDW_ADD_LDS_REGY, PO_EDW_ADD_MEM, PO_EDW_ADD_MEM_QUAD, PO_EDW_DBL_MEM_QUAD, PO_EDW_FROM_AFFINE,   // ec_edw.cuh
  PO_EDW_LOCK,                                                                                          // pre_issue, open, 0 .. 2 madd
  PO_COUNT
};
enum { PO_ROW_IN = 224, PO_ROW_OUT = 217, PO_B = 108, PO_AUX = 216, PO_FLAG = 108, PO_BOUT = 109 };

constexpr bool po_quad(int op) { return op == PO_ADD_MEM_QUAD || op == PO_DBL_MEM_QUAD || op == PO_EDW_ADD_MEM_QUAD || op == PO_EDW_DBL_MEM_QUAD; }
constexpr bool po_a_in_mem(int op) {
  return op == PO_MADD_MEM || op == PO_ADD_MEM_S || op == PO_DBL_MEM || op == PO_EDW_ADD_MEM || po_quad(op);
}
constexpr bool po_b_in_mem(int op) {
  return op == PO_ADD_LDS_REGY || op == PO_ADD_MEM_S || op == PO_ADD_MEM_QUAD || op == PO_EDW_ADD_LDS_REGY || op == PO_EDW_ADD_MEM ||
         op == PO_EDW_ADD_MEM_QUAD;
}
constexpr bool po_takes_ref(int op) { return po_a_in_mem(op) || po_b_in_mem(op) || op == PO_MADD_LDS_REGY; }
constexpr bool po_returns_flag(int op) {
  return op == PO_MADD_MEM || op == PO_MADD_LDS_REGY || op == PO_ADD_LDS_REGY || op == PO_EDW_FROM_AFFINE;
}

struct PoArgs {
  const uint32_t* in;        // n rows of PO_ROW_IN words
  uint32_t* A;               // the XYZZ array of the A operands (spill target of the LDS forms): 112 n words
  uint32_t* B;               // the XYZZ array of the B operands
  const uint32_t* pk;        // n packed operands, 72 words each
  const EdwPacked* tab;      // the lockstep run's table
  const uint32_t* ent;       // n x 3 entry words
  uint32_t* out;             // n rows of PO_ROW_OUT words
  uint32_t n;
  int mem;
};

__device__ __forceinline__ Fq po_ld(const uint32_t* w) {
  Fq v;
#pragma unroll
  for (int k = 0; k < 27; k++) v.l[k] = w[k];
  return v;
}
__device__ __forceinline__ void po_st(uint32_t* w, const Fq& v) {
#pragma unroll
  for (int k = 0; k < 27; k++) w[k] = v.l[k];
}
__device__ __forceinline__ XYZZ po_ld_xyzz(const uint32_t* w) {
  XYZZ p;
  p.X = po_ld(w); p.Y = po_ld(w + 27); p.ZZ = po_ld(w + 54); p.ZZZ = po_ld(w + 81);
  return p;
}
__device__ __forceinline__ void po_st_xyzz(uint32_t* w, const XYZZ& p) {
  po_st(w, p.X); po_st(w + 27, p.Y); po_st(w + 54, p.ZZ); po_st(w + 81, p.ZZZ);
}
// the accumulator of an LDS form, copied out word for word: the 24 packed words of X, Y from its register, the two other images
__device__ __forceinline__ void po_st_lds(uint32_t* w, const uint32_t* xs, const Fq& ty, const uint32_t* zz, const uint32_t* zzz) {
#pragma unroll
  for (int k = 0; k < 27; k++) {
    w[k] = k < 24 ? xs[k * ZK_LDS_STRIDE] : 0u;
    w[54 + k] = zz[k * ZK_LDS_STRIDE];
    w[81 + k] = zzz[k * ZK_LDS_STRIDE];
  }
  po_st(w + 27, ty);
}

template <int OP>
__global__ void __launch_bounds__(64) k_point_op(PoArgs a) {
  const uint32_t t = blockIdx.x * 64u + threadIdx.x;
  const uint32_t i = po_quad(OP) ? t >> 2 : t, q = t & 3u;
  if (i >= a.n) return;
  const uint32_t* row = a.in + (size_t)i * PO_ROW_IN;
  uint32_t* o = a.out + (size_t)i * PO_ROW_OUT;
  const bool neg = row[PO_AUX] != 0u;
  (void)q; (void)neg;
  if constexpr (OP == PO_DBL_AFFINE) {
    po_st_xyzz(o, xyzz_dbl_affine(po_ld(row + PO_B), po_ld(row + PO_B + 27)));
  } else if constexpr (OP == PO_DBL) {
    po_st_xyzz(o, xyzz_dbl(po_ld_xyzz(row)));
  } else if constexpr (OP == PO_MADD) {
    XYZZ acc = po_ld_xyzz(row);
    xyzz_madd(acc, po_ld(row + PO_B), po_ld(row + PO_B + 27));
    po_st_xyzz(o, acc);
  } else if constexpr (OP == PO_ADD) {
    XYZZ acc = po_ld_xyzz(row);
    xyzz_add(acc, po_ld_xyzz(row + PO_B));
    po_st_xyzz(o, acc);
  } else if constexpr (OP == PO_NEG) {
    XYZZ acc = po_ld_xyzz(row);
    xyzz_neg(acc);
    po_st_xyzz(o, acc);
  } else if constexpr (OP == PO_EDW_FROM_AFFINE) {
    const AffPacked* p = reinterpret_cast<const AffPacked*>(a.pk + (size_t)i * 72);
    o[PO_FLAG] = edw_from_affine(aff_ld_x(p), aff_ld_y(p, false), reinterpret_cast<EdwPacked*>(o)) ? 1u : 0u;     // as k_table_edw calls it
  } else if constexpr (po_a_in_mem(OP)) {
    const XyzzRef A = a.mem ? make_slot_ref(a.A, a.n, i) : make_ref(a.A, a.n, i);
    const XyzzRef B = a.mem ? make_slot_ref(a.B, a.n, i) : make_ref(a.B, a.n, i);
    (void)B;
    if constexpr (OP == PO_MADD_MEM) {
      o[PO_FLAG] = madd_mem(A, reinterpret_cast<const AffPacked*>(a.pk + (size_t)i * 72), neg) ? 1u : 0u;
    } else if constexpr (OP == PO_ADD_MEM_S) {
      __shared__ uint32_t s_zz[27 * ZK_LDS_STRIDE], s_zzz[27 * ZK_LDS_STRIDE];
      add_mem_s(A, B, s_zz + threadIdx.x, s_zzz + threadIdx.x);
    } else if constexpr (OP == PO_DBL_MEM) {
      dbl_mem(A);
    } else if constexpr (OP == PO_ADD_MEM_QUAD) {
      add_mem_quad(A, B, q);
    } else if constexpr (OP == PO_DBL_MEM_QUAD) {
      dbl_mem_quad(A, q);
    } else if constexpr (OP == PO_EDW_ADD_MEM) {
      edw_add_mem(A, B);
    } else if constexpr (OP == PO_EDW_ADD_MEM_QUAD) {
      edw_add_mem_quad(A, B, q);
    } else {
      static_assert(OP == PO_EDW_DBL_MEM_QUAD, "");
      edw_dbl_mem_quad(A, q);
    }
  } else {
    // the accumulator on the CU: X (packed), ZZ / Z, ZZZ / T in LDS, Y in a register
    __shared__ uint32_t lds_zz[27 * ZK_LDS_STRIDE], lds_zzz[27 * ZK_LDS_STRIDE], lds_x[24 * ZK_LDS_STRIDE];
    uint32_t* zz = lds_zz + threadIdx.x;
    uint32_t* zzz = lds_zzz + threadIdx.x;
    uint32_t* xs = lds_x + threadIdx.x;
    if constexpr (OP == PO_EDW_LOCK) {
      const EdwPacked* etab = a.tab;
      const uint32_t* entries = a.ent;
      const uint32_t cnt = row[PO_AUX + 4];
      const uint32_t trip = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt);
      const uint32_t off = 3u * i;
      Fq ty, T0, T1, T2;           // (not initialised: written before they are read)
      uint32_t e = cnt ? entries[off] : 0u;
      uint32_t e1 = cnt > 1u ? entries[off + 1u] : 0u, e2 = cnt > 2u ? entries[off + 2u] : 0u;
      if (cnt) {
        edw_pre_issue(T0, T1, T2, etab, e);
        edw_open_lds_pre(xs, zz, zzz, ty, T0, T1, T2, (e >> 31) != 0, etab, e1, cnt > 1u);
      }
      for (uint32_t j = 1; j < trip; j++) {
        if (j < cnt) {
          e = e1; e1 = e2;
          edw_madd_lds_pre(xs, zz, zzz, ty, T0, T1, T2, (e >> 31) != 0, etab, e1, j + 1 < cnt, e2, entries, off + j + 2, j + 2 < cnt);
        }
      }
      if (cnt) po_st_lds(o, xs, ty, zz, zzz);
    } else {
      lds_st_packed(xs, po_ld(row));
      Fq ty = po_ld(row + 27);
      lds_st(zz, po_ld(row + 54));
      lds_st(zzz, po_ld(row + 81));
      const XyzzRef S = a.mem ? make_slot_ref(a.A, a.n, i) : make_ref(a.A, a.n, i);       // acc / spill
      const XyzzRef B = a.mem ? make_slot_ref(a.B, a.n, i) : make_ref(a.B, a.n, i);
      (void)S; (void)B;
      if constexpr (OP == PO_MADD_LDS_REGY) {
        o[PO_FLAG] = madd_lds_regy(S, xs, zz, zzz, ty, reinterpret_cast<const AffPacked*>(a.pk + (size_t)i * 72), neg) ? 1u : 0u;
      } else if constexpr (OP == PO_ADD_LDS_REGY) {
        o[PO_FLAG] = add_lds_regy(S, xs, zz, zzz, ty, B) ? 1u : 0u;
      } else if constexpr (OP == PO_EDW_MADD_LDS_REGY) {
        edw_madd_lds_regy(xs, zz, zzz, ty, reinterpret_cast<const EdwPacked*>(a.pk + (size_t)i * 72), neg);
      } else {
        static_assert(OP == PO_EDW_ADD_LDS_REGY, "");
        edw_add_lds_regy(xs, zz, zzz, ty, B);
      }
      po_st_lds(o, xs, ty, zz, zzz);
    }
  }
}

template <int OP>
static void po_launch(const PoArgs& a) {
  const uint32_t per = po_quad(OP) ? 16u : 64u;
  hipLaunchKernelGGL(k_point_op<OP>, dim3((a.n + per - 1) / per), dim3(64), 0, 0, a);
}

int msm_point_ops_selftest(int op, int mem, const uint32_t* in_host, size_t n, const uint32_t* table_host, size_t n_table, uint32_t* out_host,
                           char* errbuf, size_t errlen) {
  auto bad = [&](const char* why) {
    if (errbuf) snprintf(errbuf, errlen, "msm_point_ops_selftest: %s (op %d, mem %d)", why, op, mem);
    return ZKHIP_ERR_ARG;
  };
  if (op < 0 || op >= PO_COUNT) return bad("unknown op");
  if (mem != 0 && !(mem == 1 && po_takes_ref(op))) return bad("mem is 0, or 1 for an op that takes a memory reference");
  if (n > (1u << 16)) return bad("at most 2^16 cases");
  if (op == PO_EDW_LOCK) {
    if (!table_host || n_table == 0 || n_table > (1u << 16)) return bad("the lockstep run needs a table of 1 .. 2^16 points");
    for (size_t i = 0; i < n; i++) {
      const uint32_t* aux = in_host + i * PO_ROW_IN + PO_AUX;
      if (aux[4] < 1 || aux[4] > 3) return bad("a run has 1 .. 3 entries");
      for (uint32_t j = 0; j < aux[4]; j++)
        if ((aux[1 + j] & 0x7fffffffu) >= n_table) return bad("an entry points past the table");
    }
  }
  if (n == 0) return ZKHIP_OK;
  // the XYZZ arrays as the references address them, laid out here with plain index arithmetic
  auto at = [&](size_t i, int c, int k) -> size_t { return mem ? i * 112 + (size_t)c * 28 + k : (size_t)(c * 27 + k) * n + i; };
  std::vector<uint32_t> hA(112 * n, 0u), hB(112 * n, 0u), hpk(72 * n), hent(3 * n), hout(n * PO_ROW_OUT, 0u);
  for (size_t i = 0; i < n; i++) {
    const uint32_t* row = in_host + i * PO_ROW_IN;
    for (int c = 0; c < 4; c++)
      for (int k = 0; k < 27; k++) {
        if (po_a_in_mem(op)) hA[at(i, c, k)] = row[c * 27 + k];
        if (po_b_in_mem(op)) hB[at(i, c, k)] = row[PO_B + c * 27 + k];
      }
    for (int k = 0; k < 72; k++) hpk[i * 72 + k] = row[PO_B + k];
    for (int j = 0; j < 3; j++) hent[i * 3 + j] = row[PO_AUX + 1 + j];
  }
  const size_t tab_words = op == PO_EDW_LOCK ? n_table * 72 : 72;
  uint32_t *d_in = nullptr, *d_A = nullptr, *d_B = nullptr, *d_pk = nullptr, *d_tab = nullptr, *d_ent = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, n * PO_ROW_IN * 4);
  if (e == hipSuccess) e = hipMalloc(&d_A, hA.size() * 4);
  if (e == hipSuccess) e = hipMalloc(&d_B, hB.size() * 4);
  if (e == hipSuccess) e = hipMalloc(&d_pk, hpk.size() * 4);
  if (e == hipSuccess) e = hipMalloc(&d_tab, tab_words * 4);
  if (e == hipSuccess) e = hipMalloc(&d_ent, hent.size() * 4);
  if (e == hipSuccess) e = hipMalloc(&d_out, hout.size() * 4);
  if (e == hipSuccess) e = hipMemcpy(d_in, in_host, n * PO_ROW_IN * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_A, hA.data(), hA.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_B, hB.data(), hB.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_pk, hpk.data(), hpk.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = op == PO_EDW_LOCK ? hipMemcpy(d_tab, table_host, tab_words * 4, hipMemcpyHostToDevice) : hipMemset(d_tab, 0, tab_words * 4);
  if (e == hipSuccess) e = hipMemcpy(d_ent, hent.data(), hent.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0, hout.size() * 4);
  if (e == hipSuccess) {
    const PoArgs a{d_in, d_A, d_B, d_pk, reinterpret_cast<const EdwPacked*>(d_tab), d_ent, d_out, (uint32_t)n, mem};
    switch (op) {
#define PO_CASE(OP) case OP: po_launch<OP>(a); break;
      PO_CASE(PO_DBL_AFFINE) PO_CASE(PO_DBL) PO_CASE(PO_MADD) PO_CASE(PO_ADD) PO_CASE(PO_NEG)
      PO_CASE(PO_MADD_MEM) PO_CASE(PO_MADD_LDS_REGY) PO_CASE(PO_ADD_LDS_REGY) PO_CASE(PO_ADD_MEM_S) PO_CASE(PO_DBL_MEM)
      PO_CASE(PO_ADD_MEM_QUAD) PO_CASE(PO_DBL_MEM_QUAD)
      PO_CASE(PO_EDW_MADD_LDS_REGY) PO_CASE(PO_EDW_ADD_LDS_REGY) PO_CASE(PO_EDW_ADD_MEM) PO_CASE(PO_EDW_ADD_MEM_QUAD)
      PO_CASE(PO_EDW_DBL_MEM_QUAD) PO_CASE(PO_EDW_FROM_AFFINE) PO_CASE(PO_EDW_LOCK)
#undef PO_CASE
      default: break;
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(hout.data(), d_out, hout.size() * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(hA.data(), d_A, hA.size() * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(hB.data(), d_B, hB.size() * 4, hipMemcpyDeviceToHost);
  uint32_t* bufs[] = {d_in, d_A, d_B, d_pk, d_tab, d_ent, d_out};
  for (uint32_t* b : bufs)
    if (b) (void)hipFree(b);
  if (e != hipSuccess) {
    if (errbuf) snprintf(errbuf, errlen, "msm_point_ops_selftest: %s", hipGetErrorString(e));
    return ZKHIP_ERR_HIP;
  }
  for (size_t i = 0; i < n; i++) {
    const uint32_t* row = in_host + i * PO_ROW_IN;
    uint32_t* o = out_host + i * PO_ROW_OUT;
    for (int k = 0; k < PO_ROW_OUT; k++) o[k] = hout[i * PO_ROW_OUT + k];
    for (int c = 0; c < 4; c++)
      for (int k = 0; k < 27; k++) {
        if (po_a_in_mem(op)) o[c * 27 + k] = hA[at(i, c, k)];
        o[PO_BOUT + c * 27 + k] = po_b_in_mem(op) ? hB[at(i, c, k)] : row[PO_B + c * 27 + k];
      }
    if (!po_returns_flag(op)) {          // a void function: does the result test as infinite / empty?
      Fq z;
      for (int k = 0; k < 27; k++) z.l[k] = o[54 + k];
      o[PO_FLAG] = fp_is_zero_2p(z) ? 1u : 0u;
    }
  }
  return ZKHIP_OK;
}

}  // namespace zkhip
