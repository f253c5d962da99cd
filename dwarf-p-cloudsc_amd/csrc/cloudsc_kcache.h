// cloudsc_kcache.h -- the CLOUDSC column physics for CDNA4 (gfx950), split into
// per-level phases, and the SCC-k-caching kernel body built from them.
//
// Semantics: the reference kernel src/cloudsc_c/cloudsc/cloudsc_c.c:19-2587
// (restated, bit-exact on the CPU, by oracle/cloudsc_oracle.c).  Structure:
// the k-caching layout of src/cloudsc_gpu/cloudsc_gpu_scc_k_caching_mod.F90 --
// an NPROMA block is one workgroup, a column is one lane, and ONE fused loop
// walks the levels top-down.  Everything the reference keeps in level-sized
// temporaries (ztp1, za, zqx, zqx0, zlneg, zqxn2d, zfoealfa, zpfplsx, ...) is
// consumed at the level that produces it, so the only state that survives an
// iteration is a handful of registers (CarryState): T/A/PAP of the level above,
// zanewm1, zqxnm1[ql,qi], zpfplsx[qi,qr,qs], zcovptot, zcovpmax, zcldtopdist,
// prainfrac, and the six running flux sums of section 8 (which the CUDA
// k-caching kernel re-reads from HBM every level, cloudsc_c_k_caching.cu:2557-2576;
// here they never leave the register file).  HBM traffic is the compulsory
// one: each input element read once, each output element written once
// (56,036 B/column in fp64).
//
// Latency hiding: only NGPTOT/64 waves exist (2560 at 163840 columns, 2.5 per
// SIMD), so the loop software-pipelines its loads: the inputs of level k+1 are
// issued before the physics of level k runs (LevelIn `nxt`), and the fields the
// physics needs one level ahead (paph, pmfu, pmfd, plu) two levels ahead.
//
// Arithmetic keeps the reference's operand order (hipcc -ffp-contract=off, so
// no FMA contraction), divisions are correctly rounded (cl_div) and fp64
// exp/pow are the reference CPU build's own algorithms (cloudsc_libm.h): the
// fp64 output is the reference kernel's, bit for bit.
#pragma once
#include "cloudsc_dev.h"
#include "cloudsc_internal.h"
#define CLOUDSC_PARAMS_HERE const PT& c = *(const PT*)launder_uniform(cpar)

namespace cloudsc {

// `real` is the type the physics computes in, `store` the element type of the
// fields in memory.  They differ only for CLOUDSC_MIXED (double arithmetic on
// float fields): a load widens (exact), a store narrows with one conversion
// (round to nearest even, gradual underflow), and everything between --
// LevelIn, Neighbors, CarryState, the parameter block, the KSEG workspace --
// is `real`.  The access helpers below are typed by the pointer they are given.
template <typename real, typename store = real>
struct KArgs {
  const store *pt, *pq, *ttt, *ttq, *tta, *ttcld, *pvfl, *pvfi, *phrsw, *phrlw, *pvervel;
  const store *pap, *paph, *plsm;
  const int *ktype;
  const store *plu, *psnde, *pmfu, *pmfd, *pa, *pclv, *psupsat, *picrit_aer, *pre_ice, *pnice;
  const store *plude_in;   // plude as read: == plude (in place, the C ABI) or a pristine copy (state runs)
  store *plude, *tlt, *tlq, *tla, *tlcld, *pcovptot, *prainfrac;
  store *pfsqlf, *pfsqif, *pfcqnng, *pfcqlng, *pfsqrf, *pfsqsf, *pfcqrng, *pfcqsng;
  store *pfsqltur, *pfsqitur, *pfplsl, *pfplsn, *pfhpsl, *pfhpsn;
  const DevParams<real>* par;   // the launch's parameter set (device memory, read with scalar loads)
  int ngptot, nproma, klev;
};
// The kernel arguments of the "tendency buffer" form (TB): the eight tendency
// members tendency_tmp_* / tendency_loc_* are planes of two packed buffers
// [nblocks][tend_planes][klev][nproma] (the reference's Fortran drivers'
// BUFFER_TMP / BUFFER_LOC), each member pointer the start of its plane in block
// 0; the block stride of these members is tend_planes * klev * nproma elements.
template <typename real, typename store = real>
struct KArgsTB : KArgs<real, store> {
  int tend_planes;
};
// The kernel arguments of the "cumulative tendency" form (CML, cloudsc_gpu_run_tendbuf_cml): KArgsTB,
// and the plane starts in block 0 of a third buffer of the same shape and block stride (the Fortran
// drivers' BUFFER_CML), to which the step adds its seven local tendencies (T, Q, A, CLD ql/qi/qr/qs)
// instead of storing them: tlt, tlq, tla and tlcld are never touched (they may be NULL), and the fifth
// (vapour) plane behind cml_cld is neither read nor written.
template <typename real, typename store = real>
struct KArgsCML : KArgsTB<real, store> {
  store *cml_t, *cml_q, *cml_a, *cml_cld;
};
// The kernel arguments of the "per-column multiplier" form (SPP, cloudsc_gpu_run_spp): the plain KArgs, and behind
// them the five multiplier fields of cloudsc_spp_t in member order -- surface fields [nblocks][nproma] of the
// storage type, read with the lane offset of plsm (lo_surf); NULL: that parameter is not perturbed.
enum { SPP_RAMID = 0, SPP_RCLDIFF = 1, SPP_RCLCRIT = 2, SPP_RLCRITSNOW = 3, SPP_RPECONS = 4, SPP_N = 5 };
template <typename real, typename store = real>
struct KArgsSPP : KArgs<real, store> {
  const store* mult[SPP_N];
};
// The kernel arguments of the "advancing" form (ADV, cloudsc_gpu_run_advance): the plain KArgs, and behind them the
// four arrays of cloudsc_advance_t, to which the step stores the updated prognostics (store_level_adv) instead of
// the local tendencies: tlt, tlq, tla and tlcld are never touched (they may be NULL).  Each array is the state
// member it advances (pt, pq, pa, pclv: in place) or another array of the same shape.
template <typename real, typename store = real>
struct KArgsADV : KArgs<real, store> {
  store *adv_t, *adv_q, *adv_a, *adv_clv;
};

// One k-caching kernel, described at compile time: the compute and storage
// types, the configuration (occupancy target WAVES, load schedule PF, aerosol
// inputs AER, carried state in LDS LDSC, float-internal exp/pow FAST) and the
// form, a set of kForm* bits:
//   kFormPack  narrow blocks packed into full waves (PackArgs, below)
//   kFormTb    the tendency buffer form (KArgsTB)
//   kFormProg  the prognostic-outputs form (flux_level)
//   kFormSurf  the surface-fluxes form (flux_surface): kFormProg, and pfplsl, pfplsn, pfhpsl, pfhpsn
//              stored once, after the last level, as surface fields
//   kFormCml   the cumulative tendency form (KArgsCML, load_cml, store_level_cml): kFormTb and kFormProg
//   kFormSpp   the per-column multiplier form (KArgsSPP, SppCol): alone or with kFormProg
//   kFormAdv   the advancing form (KArgsADV, store_level_adv): alone or with kFormProg and kFormSurf
// The kernel entries, the bodies below and the host's launch path all take the
// descriptor and read its members by name.  (The bits themselves are in cloudsc_internal.h, beside the
// support matrix that the GPU and the CPU entries share.)
template <typename Real, typename Store, int WAVES, int PF, bool AER, bool LDSC, bool FAST, unsigned FORM = 0u>
struct KForm {
  using real = Real;
  using store = Store;
  static constexpr int waves = WAVES, pf = PF;
  static constexpr bool aer = AER, ldsc = LDSC, fast = FAST;
  static constexpr bool pack = (FORM & kFormPack) != 0, tb = (FORM & kFormTb) != 0, prog = (FORM & kFormProg) != 0;
  static constexpr bool surf = (FORM & kFormSurf) != 0, cml = (FORM & kFormCml) != 0, spp = (FORM & kFormSpp) != 0;
  static constexpr bool adv = (FORM & kFormAdv) != 0;
  static_assert(!surf || prog, "the surface-fluxes form is a prognostic-outputs form");
  static_assert(!cml || (tb && prog), "the cumulative tendency form is a tendency buffer, prognostic-outputs form");
  static_assert(!spp || !(tb || surf || cml), "the per-column multiplier form stands alone or with the prognostic-outputs form");
  static_assert(!adv || (!(tb || cml || spp) && prog == surf), "the advancing form stands alone or with the surface-fluxes form");
  using fields = KArgs<real, store>;   // what the bodies read: the kernel arguments, or their base in the TB form
  // the kernel's first argument
  using kargs = typename std::conditional<
      adv, KArgsADV<real, store>,
      typename std::conditional<
          spp, KArgsSPP<real, store>,
          typename std::conditional<cml, KArgsCML<real, store>,
                                    typename std::conditional<tb, KArgsTB<real, store>, fields>::type>::type>::type>::type;
  using params = DevParamsT<real, fast, false, spp>;                                  // the parameter block
};

enum { QL = 0, QI = 1, QR = 2, QS = 3, QV = 4 };

// Field access = uniform element index (SGPR arithmetic on a uniform base
// pointer) + the lane's byte offset (one shared 32-bit VGPR).  This is the
// global_load/store "saddr" form: no per-field 64-bit VGPR pointers.
template <typename T>
CLOUDSC_HD T ldg(const T* ubase, size_t uidx, unsigned lane_bytes) {
  return *(const T*)((const char*)(ubase + uidx) + lane_bytes);
}
// Outputs are written once and never read back by the kernel, and the level
// inputs are read once: the inputs are non-temporal (streaming) loads, so the
// caches keep what is re-read (the neighbour levels, the hand-off state)
// (-1.9 % kernel time with nt loads and stores, profiles/r01/ab_nontemporal.txt).
// The outputs are write-through stores (sc1: an agent-scope relaxed atomic store
// lowers to global_store ... sc1, which leaves no line of it in the XCD's L2;
// plain and nt stores keep theirs, MI355X_MICROARCH.md): -0.7...-0.8 % fp64 and
// -0.5 % fp32 against nt stores, the same bits (profiles/r05/experiments_kernel_ab.txt).
// stg_cached is for scratch that is read back (the SCC variant's temporaries).
template <typename T>
CLOUDSC_HD void stg_cached(T* ubase, size_t uidx, unsigned lane_bytes,
                                           typename std::common_type<T>::type v) {
  *(T*)((char*)(ubase + uidx) + lane_bytes) = v;
}
#if defined(__HIP_DEVICE_COMPILE__)
// the write-through store of one output element (4 or 8 bytes, naturally aligned)
template <typename T, typename P>
__device__ __forceinline__ void st_wt(P* p, T v) {
  using U = typename std::conditional<sizeof(T) == 8, unsigned long long, unsigned>::type;
  U bits;
  __builtin_memcpy(&bits, &v, sizeof(T));
  __hip_atomic_store((U*)p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif
template <typename T>
CLOUDSC_HD void stg(T* ubase, size_t uidx, unsigned lane_bytes, typename std::common_type<T>::type v) {
#if defined(__HIP_DEVICE_COMPILE__)
  st_wt<T>((char*)(ubase + uidx) + lane_bytes, (T)v);
#else
  *(T*)((char*)(ubase + uidx) + lane_bytes) = v;
#endif
}
// a level input, read exactly once
template <typename T>
CLOUDSC_HD T ldg1(const T* ubase, size_t uidx, unsigned lane_bytes) {
  return __builtin_nontemporal_load((const T*)((const char*)(ubase + uidx) + lane_bytes));
}

// The same accesses with the uniform address made opaque first (fp32): several
// accesses of one field at different uniform indices (the species planes)
// otherwise share one 64-bit VGPR pointer, base + lane offset, and each adds its
// index to it with a VALU op; with the uniform pointer opaque, every access is
// the saddr + voffset form.  fp32 only: its level loop is VALU-issue-bound.
template <typename T>
CLOUDSC_HD T ldg1_u(const T* ubase, size_t uidx, unsigned lane_bytes) {
#if defined(__HIP_DEVICE_COMPILE__)
  const T* p = ubase + uidx;
  asm("" : "+s"(p));   // (the asm's output is a generic pointer: global address space restated below)
  using GT = const __attribute__((address_space(1))) T;
  return __builtin_nontemporal_load((GT*)((const __attribute__((address_space(1))) char*)p + lane_bytes));
#else
  return ldg1(ubase, uidx, lane_bytes);
#endif
}
template <typename T>
CLOUDSC_HD void stg_u(T* ubase, size_t uidx, unsigned lane_bytes, typename std::common_type<T>::type v) {
#if defined(__HIP_DEVICE_COMPILE__)
  T* p = ubase + uidx;
  asm("" : "+s"(p));
  st_wt<T>((__attribute__((address_space(1))) char*)p + lane_bytes, (T)v);
#else
  stg(ubase, uidx, lane_bytes, v);
#endif
}
// species planes: the opaque-pointer form in fp32, the plain one in fp64.
// Mixed (float fields, double arithmetic) has fp32's addresses and fp64's
// VALU load; which form it takes is CLOUDSC_MIXED_SP_OPAQUE.
#ifndef CLOUDSC_MIXED_SP_OPAQUE
#define CLOUDSC_MIXED_SP_OPAQUE 1
#endif
template <typename real, typename store>
constexpr bool kSpOpaque = sizeof(store) == 4 && (sizeof(real) == 4 || CLOUDSC_MIXED_SP_OPAQUE);
template <bool OPAQUE, typename T>
CLOUDSC_HD T ldg1_sp(const T* ubase, size_t uidx, unsigned lane_bytes) {
  if constexpr (OPAQUE) return ldg1_u(ubase, uidx, lane_bytes);
  else return ldg1(ubase, uidx, lane_bytes);
}
template <bool OPAQUE, typename T>
CLOUDSC_HD void stg_sp(T* ubase, size_t uidx, unsigned lane_bytes, typename std::common_type<T>::type v) {
  if constexpr (OPAQUE) stg_u(ubase, uidx, lane_bytes, v);
  else stg(ubase, uidx, lane_bytes, v);
}

// The lane's byte offset, by field kind.  Unpacked (one NPROMA block, or one
// 64-column sub-block of it, per wave) every kind has the same offset, jl *
// sizeof(S): the type is a plain `unsigned`.  Packed (a wave walks p = 64 /
// nproma consecutive blocks, lane l = s * nproma + jl serving column jl of block
// b0 + s) the uniform base is block b0's and sub-slot s is a whole block further
// on, whose size depends on the kind: PackLo keeps jl and s * nproma in bytes
// (two VGPRs) and forms each kind's offset where it is used, one multiply-add by
// a uniform factor, instead of keeping four offsets alive across the level.
struct PackLo {
  unsigned jb;   // jl * sizeof(S)
  unsigned sb;   // s * nproma * sizeof(S)
  int klev;      // uniform
};
CLOUDSC_HD unsigned lo_full(unsigned lo) { return lo; }      // [nblocks][klev][nproma]
CLOUDSC_HD unsigned lo_half(unsigned lo) { return lo; }      // [nblocks][klev+1][nproma]
CLOUDSC_HD unsigned lo_spec(unsigned lo) { return lo; }      // [nblocks][5][klev][nproma]
CLOUDSC_HD unsigned lo_surf(unsigned lo) { return lo; }      // [nblocks][nproma]
CLOUDSC_HD unsigned lo_full(const PackLo& p) { return p.sb * (unsigned)p.klev + p.jb; }
CLOUDSC_HD unsigned lo_half(const PackLo& p) { return p.sb * (unsigned)(p.klev + 1) + p.jb; }
CLOUDSC_HD unsigned lo_spec(const PackLo& p) { return p.sb * (unsigned)(5 * p.klev) + p.jb; }
CLOUDSC_HD unsigned lo_surf(const PackLo& p) { return p.sb + p.jb; }
CLOUDSC_HD PackLo launder_vgpr(PackLo p) {
  p.jb = launder_vgpr(p.jb);
  p.sb = launder_vgpr(p.sb);
  return p;
}
// A copy of the lane's values from which offsets are formed where they are used:
// offsets formed from one shared copy are loop-invariant and would be hoisted,
// one more register each live across the level loop.  The unpacked offset is
// its own only form and stays as it is.
CLOUDSC_HD unsigned lane_here(unsigned lo) { return lo; }
CLOUDSC_HD PackLo lane_here(const PackLo& p) { return launder_vgpr(p); }

// The tendency buffer form (TB) of the three functions that touch the eight
// tendency members: load_early, load_level, store_level.  Their block base in a
// buffer is ut = b * tend_planes * klev * nproma = u2 * tend_planes, formed
// where it is used from the level fields' block base u2 and the (re-laundered)
// kernel arguments, so TB adds no argument and nothing live across the level;
// the species member indexes ut + (m * klev + k) * nproma, as u3 does.  A
// packed lane's sub-slot s is s blocks of a buffer further on.  With TB off the
// functions' expressions are the ones of the fields' kinds, untouched.
template <typename real, typename S>
CLOUDSC_HD int tend_planes_of(const KArgs<real, S>& A) {
  return static_cast<const KArgsTB<real, S>&>(A).tend_planes;
}
CLOUDSC_HD unsigned lo_tend(unsigned lo, int) { return lo; }      // [nblocks][tend_planes][klev][nproma]
CLOUDSC_HD unsigned lo_tend(const PackLo& p, int tend_planes) {
  return p.sb * (unsigned)(tend_planes * p.klev) + p.jb;
}
template <typename real, typename S>
CLOUDSC_HD const KArgsCML<real, S>& cml_args_of(const KArgs<real, S>& A) {
  return static_cast<const KArgsCML<real, S>&>(A);
}

// The cumulative tendency form (CML): the seven elements of BUFFER_CML that level k of one column
// adds to, at the indices store_level forms for the local tendencies (TB); store_level_cml stores the sums.  Read once: streaming
// loads.  Where in the level they are issued is CLOUDSC_CML_AT (kcache_levels).
template <typename real>
struct CmlIn {
  real t, q, a, cld[4];
};
struct NoCml {};   // what the other forms have in its place
template <typename real, typename S, typename LO>
CLOUDSC_HD void load_cml(CmlIn<real>& C, const KArgs<real, S>& A, size_t u2, int k, int klev, int nproma, LO lane) {
  const KArgsCML<real, S>& M = cml_args_of(A);
  const int tp = M.tend_planes;
  const size_t t3 = u2 * (size_t)tp, it = t3 + (size_t)k * nproma;
  const unsigned lot = lo_tend(lane, tp);
  C.t = ldg1(M.cml_t, it, lot); C.q = ldg1(M.cml_q, it, lot); C.a = ldg1(M.cml_a, it, lot);
#pragma unroll
  for (int m = 0; m < 4; m++)
    C.cld[m] = ldg1_sp<kSpOpaque<real, S>>(M.cml_cld, t3 + ((size_t)m * klev + k) * nproma, lot);
}

// The five parameters a column may have of its own (SPP), as the physics asks for them.  NoSpp: the launch's set
// as it is -- the physics then reads the parameter block exactly as it always did.  SppCol: the set's value times
// the column's multiplier, by the contract of cloudsc_gpu_run_spp (include/cloudsc_amd.h): single operations in
// `real`, in the order of fold_params, each with its own rounding (-ffp-contract=off).  The values are per lane:
// they never pass through pval / sval.
//
// The multipliers live nowhere: each is read again where it is used -- one cached vector load per use and level from
// a field that stays in L2, issued unconditionally ahead of the branch that consumes it (no branch around a memory
// operation), no register live across the level loop.  (Carrying the four perturbed values of the level loop in
// VGPRs instead spills in the fp64 kernels with aerosol inputs: DESIGN.md 3.28 has the resource tables of both.)
// A later KSEG segment of a column forms the same values again from the same fields: the hand-off record does not
// know about them.
struct NoSpp {
  static constexpr bool on = false;
};
// the kernel arguments behind `ka`: the kernarg segment through a freshly laundered constant-space pointer on the
// device (a scalar load next to its use), the struct itself on the host
template <typename T>
CLOUDSC_HD const T& args_here(const T* ka) { return *ka; }
template <typename T>
__device__ __forceinline__ const T& args_here(cptr<T> ka) { return *(const T*)launder_uniform(ka); }
template <typename real, typename S, typename KA, typename LO>
struct SppCol {
  static constexpr bool on = true;
  KA ka;        // the kernel's KArgsSPP, as its KArgs base
  size_t u1;    // the block's base in a surface field
  LO lane;
  // the column's multiplier of one slot, widened exactly where the fields are float under double; 1 for a NULL member
  // (a uniform branch: x * 1 is x, so such a parameter has the bits of the launch's set)
  CLOUDSC_HD real mult(int slot) const {
    const S* p = static_cast<const KArgsSPP<real, S>&>(args_here(ka)).mult[slot];
    return p ? (real)ldg(p, u1, lo_surf(lane_here(lane))) : R(1.0);
  }
  template <typename P> CLOUDSC_HD real ramid(const P& c) const { return c.ramid * mult(SPP_RAMID); }
  template <typename P> CLOUDSC_HD real zldifdt0(const P& c) const {
    const real r = c.rcldiff * mult(SPP_RCLDIFF);
    return r * c.ptsphy;
  }
  // (not read where the aerosol value replaces it)
  template <typename P> CLOUDSC_HD real rlcritsnow(const P& c) const {
    return c.laericeauto ? R(0.0) : c.rlcritsnow * mult(SPP_RLCRITSNOW);
  }
  template <typename P> CLOUDSC_HD real rg_rpecons(const P& c) const { return c.rg * (c.rpecons * mult(SPP_RPECONS)); }
};

// Per-level inputs of one column (the prefetch unit).
template <typename real>
struct LevelIn {
  real pt, pq, ttt, ttq, tta, pa, pap, phrsw, phrlw, pvervel, plude, psnde, psupsat, pvfl, pvfi;
  real pclv[4], ttcld[4];
  real pre_ice, picrit_aer, pnice;      // aerosol inputs, loaded only under LAERICESED/LAERICEAUTO
};

// PF 3: the inputs section 1 and the start of section 3 consume first
// (init_level, the saturation values), prefetched for level k+1 in the middle
// of level k; the rest is loaded at the top of its own level.
template <typename real>
struct EarlyIn {
  real pt, pq, ttt, ttq, tta, pa, pap;
  real pclv[4], ttcld[4];
};
template <typename real, bool TB = false, typename S, typename LO>
CLOUDSC_HD void load_early(EarlyIn<real>& E, const KArgs<real, S>& A, size_t u2, size_t u3, int k, int klev,
                           int nproma, LO lane) {
  const size_t i = u2 + (size_t)k * nproma;
  const unsigned lo = lo_full(lane), ls = lo_spec(lane);
  size_t it = i, t3 = u3;            // the tendency members' level index, species base and lane offsets
  unsigned lot = lo, lst = ls;
  if constexpr (TB) {
    const int tp = tend_planes_of(A);
    t3 = u2 * (size_t)tp;
    it = t3 + (size_t)k * nproma;
    lot = lst = lo_tend(lane, tp);
  }
  E.pt = ldg1(A.pt, i, lo); E.pq = ldg1(A.pq, i, lo); E.ttt = ldg1(A.ttt, it, lot); E.ttq = ldg1(A.ttq, it, lot);
  E.tta = ldg1(A.tta, it, lot); E.pa = ldg1(A.pa, i, lo); E.pap = ldg1(A.pap, i, lo);
#pragma unroll
  for (int m = 0; m < 4; m++) {
    const size_t j = u3 + ((size_t)m * klev + k) * nproma;
    size_t jt = j;
    if constexpr (TB) jt = t3 + ((size_t)m * klev + k) * nproma;
    E.pclv[m] = ldg1_sp<kSpOpaque<real, S>>(A.pclv, j, ls);
    E.ttcld[m] = ldg1_sp<kSpOpaque<real, S>>(A.ttcld, jt, lst);
  }
}
template <typename real, bool AER, typename S, typename LO>
CLOUDSC_HD void load_late(LevelIn<real>& L, const KArgs<real, S>& A, size_t u2, int k, int nproma, LO lane) {
  const size_t i = u2 + (size_t)k * nproma;
  const unsigned lo = lo_full(lane);
  L.plude = ldg1(A.plude_in, i, lo); L.pvfl = ldg1(A.pvfl, i, lo); L.pvfi = ldg1(A.pvfi, i, lo);
  L.phrsw = ldg1(A.phrsw, i, lo); L.phrlw = ldg1(A.phrlw, i, lo); L.pvervel = ldg1(A.pvervel, i, lo);
  L.psnde = ldg1(A.psnde, i, lo); L.psupsat = ldg1(A.psupsat, i, lo);
  if (AER) {
    L.pre_ice = ldg1(A.pre_ice, i, lo); L.picrit_aer = ldg1(A.picrit_aer, i, lo); L.pnice = ldg1(A.pnice, i, lo);
  } else {
    L.pre_ice = R(0.0); L.picrit_aer = R(1.0); L.pnice = R(1.0);
  }
}
template <typename real>
CLOUDSC_HD void take_early(LevelIn<real>& L, const EarlyIn<real>& E) {
  L.pt = E.pt; L.pq = E.pq; L.ttt = E.ttt; L.ttq = E.ttq; L.tta = E.tta; L.pa = E.pa; L.pap = E.pap;
#pragma unroll
  for (int m = 0; m < 4; m++) { L.pclv[m] = E.pclv[m]; L.ttcld[m] = E.ttcld[m]; }
}

// Values of the neighbouring levels the physics of level k reads.
template <typename real>
struct Neighbors {
  real paph_k, paph_n;                  // paph(k), paph(k+1)
  real pmfu_k, pmfd_k, pmfu_n, pmfd_n;  // mass fluxes at k and k+1
  real plu_n;                           // plu(k+1)
};

// Column constants.
template <typename real>
struct ColConst {
  real paph_sfc, kk_const, kk_lcrit, kk_pow;
  int ktype;
};

// State carried from level k to level k+1.
template <typename real>
struct CarryState {
  real t_prev, a_prev, pap_prev, zanewm1, zcovptot, zcovpmax, zcldtopdist, rainfrac;
  real qxnm1_l, qxnm1_i;                // zqxnm1 of the non-falling condensates
  real pfx_i, pfx_r, pfx_s;             // zpfplsx[qi,qr,qs] arriving at level k
  real fl_lf, fl_if, fl_lng, fl_nng, fl_ltur, fl_itur;  // running flux sums (section 8)
};

// The same 19 values kept in LDS instead of registers: every wave owns 19
// planes of 64 lanes ([wave][slot][lane], conflict-free, constant ds offsets).
// They are touched a few times per level each, and taking them out of the
// register file is what lets the fp64 kernel fit more waves per SIMD.
// Accesses are volatile so that the compiler re-reads at each use instead of
// keeping a register copy alive across the level.
#define CLOUDSC_AS3 __attribute__((address_space(3)))
template <typename real, int Q>
struct LdsSlot {
  CLOUDSC_AS3 real* base;               // this lane's slot 0
  __device__ __forceinline__ operator real() const { return *(volatile CLOUDSC_AS3 real*)(base + Q * 64); }
  __device__ __forceinline__ LdsSlot& operator=(real v) {
    *(volatile CLOUDSC_AS3 real*)(base + Q * 64) = v;
    return *this;
  }
  __device__ __forceinline__ LdsSlot& operator=(const LdsSlot& o) { return *this = (real)o; }
};
template <typename real>
struct CarryLds {
  static constexpr int kSlots = 19;
  __device__ __forceinline__ explicit CarryLds(CLOUDSC_AS3 real* b)
      : t_prev{b}, a_prev{b}, pap_prev{b}, zanewm1{b}, zcovptot{b}, zcovpmax{b}, zcldtopdist{b}, rainfrac{b},
        qxnm1_l{b}, qxnm1_i{b}, pfx_i{b}, pfx_r{b}, pfx_s{b}, fl_lf{b}, fl_if{b}, fl_lng{b}, fl_nng{b},
        fl_ltur{b}, fl_itur{b} {}
  LdsSlot<real, 0> t_prev; LdsSlot<real, 1> a_prev; LdsSlot<real, 2> pap_prev; LdsSlot<real, 3> zanewm1;
  LdsSlot<real, 4> zcovptot; LdsSlot<real, 5> zcovpmax; LdsSlot<real, 6> zcldtopdist; LdsSlot<real, 7> rainfrac;
  LdsSlot<real, 8> qxnm1_l; LdsSlot<real, 9> qxnm1_i;
  LdsSlot<real, 10> pfx_i; LdsSlot<real, 11> pfx_r; LdsSlot<real, 12> pfx_s;
  LdsSlot<real, 13> fl_lf; LdsSlot<real, 14> fl_if; LdsSlot<real, 15> fl_lng; LdsSlot<real, 16> fl_nng;
  LdsSlot<real, 17> fl_ltur; LdsSlot<real, 18> fl_itur;
};
// LDS bytes of the carried state for a workgroup of nproma lanes
template <typename real>
constexpr size_t carry_lds_bytes(int nproma) {
  return (size_t)((nproma + 63) / 64) * CarryLds<real>::kSlots * 64 * sizeof(real);
}
template <typename real>
__device__ __forceinline__ CLOUDSC_AS3 real* carry_lds_base() {
  extern __shared__ __attribute__((aligned(16))) char cloudsc_dyn_lds[];
  const int t = threadIdx.x;
  return (CLOUDSC_AS3 real*)(CLOUDSC_AS3 char*)cloudsc_dyn_lds + (t >> 6) * (CarryLds<real>::kSlots * 64) + (t & 63);
}

// Result of section 1 at one level (the reference's level-sized temporaries).
template <typename real>
struct LevelState {
  real ztp1, za, zaorig, zfoealfa, ttend, qtend;
  real zqx[5], zqx0[5], zlneg[4];
};

// Result of the physics at one level.
template <typename real>
struct PhysOut {
  real zqxn[4];                         // zqxn2d(k), zero above NCLDTOP
  real plude_k, atend, ctend[4], zcovptot_out;
};

// All loads of a level are unconditional (the physics-only fields are read at
// every level): branches around memory operations make hipcc's vmcnt
// bookkeeping fall back to vmcnt(0), which drains the software pipeline.
template <typename real, bool AER, bool TB = false, typename S, typename LO>
CLOUDSC_HD void load_level(LevelIn<real>& L, const KArgs<real, S>& A, size_t u2, size_t u3, int k,
                                           int klev, int nproma, LO lane) {
  const size_t i = u2 + (size_t)k * nproma;
  const unsigned lo = lo_full(lane), ls = lo_spec(lane);
  size_t it = i, t3 = u3;            // the tendency members' level index, species base and lane offsets
  unsigned lot = lo, lst = ls;
  if constexpr (TB) {
    const int tp = tend_planes_of(A);
    t3 = u2 * (size_t)tp;
    it = t3 + (size_t)k * nproma;
    lot = lst = lo_tend(lane, tp);
  }
  L.pt = ldg1(A.pt, i, lo); L.pq = ldg1(A.pq, i, lo); L.ttt = ldg1(A.ttt, it, lot); L.ttq = ldg1(A.ttq, it, lot);
  L.tta = ldg1(A.tta, it, lot); L.pa = ldg1(A.pa, i, lo); L.pap = ldg1(A.pap, i, lo);
  L.plude = ldg1(A.plude_in, i, lo); L.pvfl = ldg1(A.pvfl, i, lo); L.pvfi = ldg1(A.pvfi, i, lo);
#pragma unroll
  for (int m = 0; m < 4; m++) {
    const size_t j = u3 + ((size_t)m * klev + k) * nproma;
    size_t jt = j;
    if constexpr (TB) jt = t3 + ((size_t)m * klev + k) * nproma;
    L.pclv[m] = ldg1_sp<kSpOpaque<real, S>>(A.pclv, j, ls);
    L.ttcld[m] = ldg1_sp<kSpOpaque<real, S>>(A.ttcld, jt, lst);
  }
  L.phrsw = ldg1(A.phrsw, i, lo); L.phrlw = ldg1(A.phrlw, i, lo); L.pvervel = ldg1(A.pvervel, i, lo);
  L.psnde = ldg1(A.psnde, i, lo); L.psupsat = ldg1(A.psupsat, i, lo);
  if (AER) {   // LAERICESED / LAERICEAUTO inputs; the launch picks AER from the flags
    L.pre_ice = ldg1(A.pre_ice, i, lo); L.picrit_aer = ldg1(A.picrit_aer, i, lo); L.pnice = ldg1(A.pnice, i, lo);
  } else {
    L.pre_ice = R(0.0); L.picrit_aer = R(1.0); L.pnice = R(1.0);
  }
}

// ===== 1. initial values, tidy-up, FOEALFA at one level (cloudsc_c.c:462-575, 588, 625) =====
template <typename real, typename P>
CLOUDSC_HD void init_level(const P& c, const LevelIn<real>& in, LevelState<real>& s) {
  s.ztp1 = in.pt + c.ptsphy * in.ttt;
  real* zqx = s.zqx;
  real* zlneg = s.zlneg;
  zqx[QV] = in.pq + c.ptsphy * in.ttq;
  s.zqx0[QV] = zqx[QV];
  real za = in.pa + c.ptsphy * in.tta;
  s.zaorig = za;
#pragma unroll
  for (int m = 0; m < 4; m++) {
    zqx[m] = in.pclv[m] + c.ptsphy * in.ttcld[m];
    s.zqx0[m] = zqx[m];
    zlneg[m] = R(0.0);
  }
  // The zero is opaque to the optimiser: with it visible, the fp32 SCC build
  // (packed v_pk_mul_f32 operands) folded (0 - a) - b into (-a) - b, which is
  // -0 instead of +0 when a = b = 0 -- a sign-of-zero change the IEEE
  // semantics (no nsz flag) do not allow.
  real ttend = launder_vgpr(R(0.0)), qtend = launder_vgpr(R(0.0));
  // tidy up very small cloud cover or total cloud water (:519-541)
  if (zqx[QL] + zqx[QI] < c.rlmin || za < c.ramin) {
    real zqadj;
    zlneg[QL] = zlneg[QL] + zqx[QL];
    zqadj = zqx[QL] * c.zqtmst;
    qtend = qtend + zqadj;
    ttend = ttend - c.ralvdcp * zqadj;
    zqx[QV] = zqx[QV] + zqx[QL];
    zqx[QL] = R(0.0);
    zlneg[QI] = zlneg[QI] + zqx[QI];
    zqadj = zqx[QI] * c.zqtmst;
    qtend = qtend + zqadj;
    ttend = ttend - c.ralsdcp * zqadj;
    zqx[QV] = zqx[QV] + zqx[QI];
    zqx[QI] = R(0.0);
    za = R(0.0);
  }
  // tidy up small CLV variables (:547-575)
#pragma unroll
  for (int m = 0; m < 4; m++) {
    if (zqx[m] < c.rlmin) {
      zlneg[m] = zlneg[m] + zqx[m];
      const real zqadj = zqx[m] * c.zqtmst;
      qtend = qtend + zqadj;
      if (m == QL || m == QR) ttend = ttend - c.ralvdcp * zqadj;   // iphase 1
      else ttend = ttend - c.ralsdcp * zqadj;                        // iphase 2
      zqx[QV] = zqx[QV] + zqx[m];
      zqx[m] = R(0.0);
    }
  }
  s.zfoealfa = foealfa<real>(c, s.ztp1);
  s.za = fmax(R(0.0), fmin(R(1.0), za));    // clip cloud fraction (:625)
  s.ttend = ttend;
  s.qtend = qtend;
}

// Per-phase cost ablation (timing-only experiment builds, tools/ablation.sh):
// -DCLOUDSC_ABLATE=<mask> skips the marked sections of the physics; the loads
// and stores stay, downstream sections see zero contributions (or, for the
// Newton chain, a cheap stand-in of the same sign), so the difference to the
// full kernel is the section's cost.  0 (the default) compiles nothing out.
#ifndef CLOUDSC_ABLATE
#define CLOUDSC_ABLATE 0
#endif
enum AblateBit : unsigned {
  AB_SUPSAT = 1u << 0,     // 3.1 supersaturation adjustment
  AB_CONV = 1u << 1,       // 3.2 detrainment, 3.3 subsidence source and sink
  AB_EROSION = 1u << 2,    // 3.4 erosion
  AB_NEWTON = 1u << 3,     // 3.4 dqs/dt: the two Newton steps
  AB_COND = 1u << 4,       // 3.4a/b evaporation, condensation, new clouds
  AB_DEPOS = 1u << 5,      // 3.7 ice deposition
  AB_SEDIM = 1u << 6,      // 4.2 sedimentation, precipitation cover
  AB_AUTO = 1u << 7,       // 4.3 autoconversion (snow, KK rain), riming
  AB_MELT = 1u << 8,       // 4.4 melting, freezing
  AB_EVAP = 1u << 9,       // 4.5 rain and snow evaporation
  AB_TRUNC = 1u << 10,     // 5.2 sink truncation
  AB_SOLVE = 1u << 11,     // 5.2.2 implicit solver (divisions and substitutions)
  AB_SAT = 1u << 12,       // saturation exponentials at T (e_liq, e_ice): cheap stand-ins
};
constexpr unsigned kAblate = CLOUDSC_ABLATE;
#define CLOUDSC_RUN(bit) ((kAblate & (bit)) == 0)

// ===== 3.-6. physics of one level ncldtop <= k (cloudsc_c.c:732-2508) =====
// Where in the level physics_level calls its mid hook: 0 (the default) after
// 5.1; experiment builds (VFLAGS=-DCLOUDSC_MID_AT=n) move it earlier -- 1 before
// the Newton steps of 3.4, 2 before 3.7, 3 before 4.2, 4 before 4.4, 5 before
// 4.5 -- trading a longer flight time of the next level's loads against their
// registers being live across more of the physics.
#ifndef CLOUDSC_MID_AT
#define CLOUDSC_MID_AT 0
#endif
#define CLOUDSC_MID_HOOK(n) do { if constexpr (CLOUDSC_MID_AT == (n)) mid(); } while (0)
// Nothing to do at the middle of a level (the default hook of physics_level).
struct NoMidHook {
  CLOUDSC_HD void operator()() const {}
};

#define CLOUDSC_PHYSICS_SPP 0
#include "cloudsc_physics_level.inc"
#undef CLOUDSC_PHYSICS_SPP
#define CLOUDSC_PHYSICS_SPP 1
#include "cloudsc_physics_level.inc"
#undef CLOUDSC_PHYSICS_SPP

// ===== 8. flux diagnostics of one level (cloudsc_c.c:2521-2582), written at half level k+1 =====
// PROG: the prognostic-outputs form (cloudsc_gpu_run_outputs, CLOUDSC_OUTPUTS_PROGNOSTIC).  The ten
// diagnostic fluxes pfsqlf ... pfsqitur are running sums that nothing in the step reads back: with
// PROG on they are neither computed nor stored, their six carried sums (fl_* of the carried state)
// are never touched -- not initialised, not carried, not handed over between KSEG segments -- and
// their members of the kernel arguments are never read (they may be NULL).  What stays is what
// pfplsl, pfplsn, pfhpsl and pfhpsn need.  With PROG off the functions are the ones they were.
// SURF (with PROG): the surface-fluxes form (CLOUDSC_OUTPUTS_SURFACE).  The four remaining profiles are
// not stored per level either -- flux_level and flux_top are empty -- and their last row is stored once,
// after the last level, from the carried precipitation fluxes (flux_surface).
template <bool PROG = false, bool SURF = false, typename real, typename P, typename CS, typename S, typename LO>
CLOUDSC_HD void flux_level(const P& c, const KArgs<real, S>& A, size_t h, LO lane,
                                           const LevelIn<real>& in, const LevelState<real>& ls,
                                           const PhysOut<real>& po, real paph_k, real paph_n,
                                           CS& cs) {
  if constexpr (!PROG) {
    const real zgdph_r = -c.zrg_r * (paph_n - paph_k) * c.zqtmst;
    const real lf = cs.fl_lf, fi = cs.fl_if, lng = cs.fl_lng, nng = cs.fl_nng;
    const real* zqxn = po.zqxn;
    const real* zqx0 = ls.zqx0;
    const real* zlneg = ls.zlneg;
    const real plude_k = po.plude_k, zfoealfa = ls.zfoealfa;
    cs.fl_lf = lf + (zqxn[QL] - zqx0[QL] + in.pvfl * c.ptsphy - zfoealfa * plude_k) * zgdph_r;
    cs.fl_lng = lng + zlneg[QL] * zgdph_r;
    cs.fl_ltur = cs.fl_ltur + (in.pvfl * c.ptsphy) * zgdph_r;
    const real rf = lf + (zqxn[QR] - zqx0[QR]) * zgdph_r;
    const real rng = lng + zlneg[QR] * zgdph_r;
    cs.fl_if = fi + (zqxn[QI] - zqx0[QI] + in.pvfi * c.ptsphy - (R(1.0) - zfoealfa) * plude_k) * zgdph_r;
    cs.fl_nng = nng + zlneg[QI] * zgdph_r;
    cs.fl_itur = cs.fl_itur + (in.pvfi * c.ptsphy) * zgdph_r;
    const real sf = fi + (zqxn[QS] - zqx0[QS]) * zgdph_r;
    const real sng = nng + zlneg[QS] * zgdph_r;
    const unsigned lo = lo_half(lane);
    stg(A.pfsqlf, h, lo, cs.fl_lf); stg(A.pfsqif, h, lo, cs.fl_if);
    stg(A.pfcqlng, h, lo, cs.fl_lng); stg(A.pfcqnng, h, lo, cs.fl_nng);
    stg(A.pfsqltur, h, lo, cs.fl_ltur); stg(A.pfsqitur, h, lo, cs.fl_itur);
    stg(A.pfsqrf, h, lo, rf); stg(A.pfcqrng, h, lo, rng); stg(A.pfsqsf, h, lo, sf); stg(A.pfcqsng, h, lo, sng);
  }
  if constexpr (!SURF) {
    const unsigned lo = lo_half(lane);
    const real plsl = cs.pfx_r + R(0.0);      // zpfplsx[qr] + zpfplsx[ql] (ql flux is +0)
    const real plsn = cs.pfx_s + cs.pfx_i;
    stg(A.pfplsl, h, lo, plsl); stg(A.pfplsn, h, lo, plsn);
    stg(A.pfhpsl, h, lo, -c.rlvtt * plsl); stg(A.pfhpsn, h, lo, -c.rlstt * plsn);
  }
}

// SURF: row klev of pfplsl, pfplsn, pfhpsl, pfhpsn -- what flux_level stores at half level klev, from the
// precipitation fluxes the last level left in the carried state -- into the members as surface fields
// ([nblocks][nproma], u1 the block's base as for prainfrac).  Called once per column after the last
// level, outside the level loop: it reads only what the carried state holds there anyway.
template <typename real, typename P, typename CS, typename S, typename LO>
CLOUDSC_HD void flux_surface(const P& c, const KArgs<real, S>& A, size_t u1, LO lane, const CS& cs) {
  const unsigned lo = lo_surf(lane);
  const real plsl = cs.pfx_r + R(0.0);      // as flux_level
  const real plsn = cs.pfx_s + cs.pfx_i;
  stg(A.pfplsl, u1, lo, plsl); stg(A.pfplsn, u1, lo, plsn);
  stg(A.pfhpsl, u1, lo, -c.rlvtt * plsl); stg(A.pfhpsn, u1, lo, -c.rlstt * plsn);
}

// level-0 half-level outputs (cloudsc_c.c:2523-2543, 2578-2579)
template <bool PROG = false, bool SURF = false, typename real, typename P, typename S, typename LO>
CLOUDSC_HD void flux_top(const P& c, const KArgs<real, S>& A, size_t h0, LO lane) {
  const unsigned lo = lo_half(lane);
  if constexpr (!PROG) {
    stg(A.pfsqlf, h0, lo, R(0.0)); stg(A.pfsqif, h0, lo, R(0.0)); stg(A.pfsqrf, h0, lo, R(0.0));
    stg(A.pfsqsf, h0, lo, R(0.0)); stg(A.pfcqlng, h0, lo, R(0.0)); stg(A.pfcqnng, h0, lo, R(0.0));
    stg(A.pfcqrng, h0, lo, R(0.0)); stg(A.pfcqsng, h0, lo, R(0.0));
    stg(A.pfsqltur, h0, lo, R(0.0)); stg(A.pfsqitur, h0, lo, R(0.0));
  }
  if constexpr (!SURF) {
    const real plsl = R(0.0) + R(0.0), plsn = R(0.0) + R(0.0);
    stg(A.pfplsl, h0, lo, plsl); stg(A.pfplsn, h0, lo, plsn);
    stg(A.pfhpsl, h0, lo, -c.rlvtt * plsl); stg(A.pfhpsn, h0, lo, -c.rlstt * plsn);
  }
}

template <typename real, typename P, typename S, typename LO>
CLOUDSC_HD ColConst<real> column_constants(const P& c, const KArgs<real, S>& A,
                                                           size_t u1, size_t uh, LO lane) {
  ColConst<real> cc;
  const unsigned lo = lo_surf(lane);
  const real plsm = ldg(A.plsm, u1, lo);
  cc.ktype = ldg(A.ktype, u1, lo * (unsigned)(sizeof(int)) / (unsigned)sizeof(S));
  cc.paph_sfc = ldg(A.paph, uh + (size_t)A.klev * A.nproma, lo_half(lane));
  const bool land = plsm > R(0.5);
  cc.kk_const = land ? pval(c, c.rcl_kk_cloud_num_land) : pval(c, c.rcl_kk_cloud_num_sea);
  cc.kk_lcrit = land ? pval(c, c.rclcrit_land) : pval(c, c.rclcrit_sea);
  cc.kk_pow = cl_pow<real>(c, cc.kk_const, c.rcl_kkbaun);   // loop-invariant factor of the KK autoconversion (:1721)
  return cc;
}

template <bool TB = false, typename real, typename S, typename LO>
CLOUDSC_HD void store_level(const KArgs<real, S>& A, size_t u2, size_t u3, int k, int klev,
                                            int nproma, LO lane, bool physics, const LevelState<real>& ls,
                                            const PhysOut<real>& po) {
  const size_t i = u2 + (size_t)k * nproma;
  const unsigned lo = lo_full(lane);
  unsigned lsp = lo_spec(lane);
  size_t it = i, t3 = u3;
  unsigned lot = lo;
  if constexpr (TB) {
    const int tp = tend_planes_of(A);
    t3 = u2 * (size_t)tp;
    it = t3 + (size_t)k * nproma;
    lot = lsp = lo_tend(lane, tp);
  }
  stg(A.tlt, it, lot, ls.ttend);
  stg(A.tlq, it, lot, ls.qtend);
  stg(A.tla, it, lot, po.atend);
  stg(A.pcovptot, i, lo, po.zcovptot_out);
  stg(A.plude, i, lo, po.plude_k);   // INOUT: rewritten unchanged where not rescaled (no branch on a store)
#pragma unroll
  for (int m = 0; m < 4; m++)
    stg_sp<kSpOpaque<real, S>>(A.tlcld, t3 + ((size_t)m * klev + k) * nproma, lsp, po.ctend[m]);
  stg_sp<kSpOpaque<real, S>>(A.tlcld, t3 + ((size_t)4 * klev + k) * nproma, lsp, R(0.0));
}

// store_level of the cumulative tendency form (CML, always with TB).  The seven local tendencies are
// not stored: each is added to the element of BUFFER_CML that load_cml read for it (`cm`) -- one add in
// `real`, its own rounding (-ffp-contract=off), narrowed by the store where the fields are float under
// double -- and the sum stored there with the outputs' write-through policy.  tlt, tlq, tla and tlcld
// are not touched; the vapour plane of CML, whose local tendency is identically zero, neither.
template <typename real, typename S, typename LO>
CLOUDSC_HD void store_level_cml(const KArgs<real, S>& A, size_t u2, int k, int klev, int nproma, LO lane,
                                const LevelState<real>& ls, const PhysOut<real>& po, const CmlIn<real>& cm) {
  const KArgsCML<real, S>& M = cml_args_of(A);
  const size_t i = u2 + (size_t)k * nproma;
  const unsigned lo = lo_full(lane);
  const int tp = M.tend_planes;
  const size_t t3 = u2 * (size_t)tp, it = t3 + (size_t)k * nproma;
  const unsigned lot = lo_tend(lane, tp);
  stg(M.cml_t, it, lot, cm.t + ls.ttend);
  stg(M.cml_q, it, lot, cm.q + ls.qtend);
  stg(M.cml_a, it, lot, cm.a + po.atend);
  stg(A.pcovptot, i, lo, po.zcovptot_out);
  stg(A.plude, i, lo, po.plude_k);   // as store_level
#pragma unroll
  for (int m = 0; m < 4; m++)
    stg_sp<kSpOpaque<real, S>>(M.cml_cld, t3 + ((size_t)m * klev + k) * nproma, lot, cm.cld[m] + po.ctend[m]);
}

// store_level of the advancing form (ADV).  The seven local tendencies are not stored: each advances the value the
// step started from, X_new = X0 + ptsphy * loc -- one multiply and one add in `real`, each with its own rounding
// (-ffp-contract=off), narrowed by the store where the fields are float under double -- and X_new is stored to the
// form's own array with the outputs' write-through policy.  X0 = X + ptsphy * tendency_tmp is what init_level formed
// and nothing since has changed: ztp1 (the Newton steps of 3.4 work on a scalar of their own), zqx0[QV] and
// zqx0[ql..qs] (the tidy-up works on zqx) and zaorig (taken before the tidy-up and the clipping of za); physics_level
// reads all of them through const copies.  tlt, tlq, tla and tlcld are not touched; the vapour plane behind adv_clv,
// whose tendency is identically zero, neither.
//
// In place (adv_x == the state member x).  A state element [b][k][jl] is read by exactly one lane, the one that
// owns column (b, jl), and only as part of that column's level k inputs (load_level, load_early: pt, pq, pa and
// pclv at row k; what level k needs of level k - 1 -- t_prev, a_prev -- travels in the carried state, never through
// memory); the same lane is the only one that stores it, here, with a value computed from that very load.  So the
// store follows its element's one consumed load by data dependence, in every load schedule:
//   PF 0, 2   row k is loaded at the top of level k and stored at its end;
//   PF 1, 4   row k + 1 is in flight while level k computes and stores row k: another element.  At the last level
//             the clamped prefetch re-reads row klev - 1 before that row's store; its value is never consumed;
//   PF 3      the same with the early inputs of row k + 1 issued in the middle of level k;
//   KSEG      a segment [lev0, lev1) loads rows lev0 .. lev1 (row lev1 by the last level's prefetch, never
//             consumed) and stores rows lev0 .. lev1 - 1; the next segment of the column starts after the hand-off
//             and loads rows >= lev1, which no earlier segment has stored.  The hand-off record carries t_prev and
//             a_prev of row lev1 - 1 as computed, not as re-read;
//   packed    a lane serves one column of one block of its group throughout: the argument holds lane by lane.
// No other lane, wave or workgroup reads or writes the element, so there is no ordering to keep across lanes, and
// a later launch on the same stream (the next time step) sees the stores as it sees any output.
template <typename real, typename S>
CLOUDSC_HD const KArgsADV<real, S>& adv_args_of(const KArgs<real, S>& A) {
  return static_cast<const KArgsADV<real, S>&>(A);
}
template <typename real, typename P, typename S, typename LO>
CLOUDSC_HD void store_level_adv(const P& c, const KArgs<real, S>& A, size_t u2, size_t u3, int k, int klev, int nproma,
                                LO lane, const LevelState<real>& ls, const PhysOut<real>& po) {
  const KArgsADV<real, S>& V = adv_args_of(A);
  const size_t i = u2 + (size_t)k * nproma;
  const unsigned lo = lo_full(lane), lsp = lo_spec(lane);
  const real dt = c.ptsphy;
  const real dtt = dt * ls.ttend, dtq = dt * ls.qtend, dta = dt * po.atend;
  stg(V.adv_t, i, lo, ls.ztp1 + dtt);
  stg(V.adv_q, i, lo, ls.zqx0[QV] + dtq);
  stg(V.adv_a, i, lo, ls.zaorig + dta);
  stg(A.pcovptot, i, lo, po.zcovptot_out);
  stg(A.plude, i, lo, po.plude_k);   // as store_level
#pragma unroll
  for (int m = 0; m < 4; m++) {
    const real dtc = dt * po.ctend[m];
    stg_sp<kSpOpaque<real, S>>(V.adv_clv, u3 + ((size_t)m * klev + k) * nproma, lsp, ls.zqx0[m] + dtc);
  }
}

template <typename real, bool PROG = false, typename CS>
CLOUDSC_HD void init_carry(CS& cs) {
  cs.t_prev = cs.a_prev = cs.pap_prev = R(0.0);
  cs.zanewm1 = cs.zcovptot = cs.zcovpmax = cs.zcldtopdist = cs.rainfrac = R(0.0);
  cs.qxnm1_l = cs.qxnm1_i = R(0.0);
  cs.pfx_i = cs.pfx_r = cs.pfx_s = R(0.0);
  if constexpr (!PROG) cs.fl_lf = cs.fl_if = cs.fl_lng = cs.fl_nng = cs.fl_ltur = cs.fl_itur = R(0.0);
}

// The level loop's parameter block: the VGPR copy (fp32) or the constant-space
// block read with scalar loads (laundered: loads issued where used).
template <bool PVR, typename PV, typename PT>
__device__ __forceinline__ const auto& params_here(const PV& pv, cptr<PT> cpar) {
  if constexpr (PVR) return pv;
  else return *(const PT*)launder_uniform(cpar);
}

// ===================== SCC-k-caching kernel body =====================
// `ka` points at the kernel's KArgs in the kernarg segment and `cpar` at the
// __constant__ parameter block, both in the constant address space; they are
// re-laundered every level so that scalar loads are issued where needed.
// PF selects the load schedule: 1 = level k+1 prefetched into registers while
// level k computes; 0 = loads issued at the top of their own level.
//
// kcache_levels runs levels [lev0, lev1) of block b for one (active) lane with
// the carried state `cs`; the plain kernel runs [0, klev) in one go, the
// persistent kernel (below) runs a column in level segments.
//
// F: the kernel's descriptor (KForm).  F::tb: the tendency buffer form (`ka`
// then points at a KArgsTB); F::prog: the prognostic-outputs form (flux_level); F::surf: the
// surface-fluxes form (flux_level stores nothing; the caller stores the surface row, flux_surface);
// F::cml: the cumulative tendency form (`ka` points at a KArgsCML; load_cml, store_level_cml);
// F::spp: the per-column multiplier form (`ka` points at a KArgsSPP; SppCol);
// F::adv: the advancing form (`ka` points at a KArgsADV; store_level_adv).
//
// Where F::cml issues the seven BUFFER_CML loads of level k (CLOUDSC_CML_AT): 2 = at the top of the
// level, behind the level's own loads; 1 = in the middle of the level (the physics' mid hook), ahead
// of the next level's early inputs; 0 = just before the stores that consume them.  The product is
// the earliest that leaves every kernel of the form without scratch and without VGPR spills at two
// waves per SIMD (profiles/tendbuf_cml/kernel_resources.txt); experiment builds override it
// (make variant VFLAGS=-DCLOUDSC_CML_AT=n).
#ifndef CLOUDSC_CML_AT
#define CLOUDSC_CML_AT 2
#endif
template <typename F, typename CS, typename LO>
__device__ __forceinline__ void kcache_levels(cptr<typename F::fields> ka, cptr<typename F::params> cpar, int b,
                                              LO lo0, int lev0, int lev1, CS& cs) {
  using real = typename F::real;
  using S = typename F::store;
  using PT = typename F::params;
  constexpr int PF = F::pf;
  constexpr bool AER = F::aer;
  if (lev0 >= lev1) return;
  const LO lo = lane_here(lo0);                        // empty segment: no loads at lev0 (may be == klev)
  // PF: 0 = loads at the top of their level, 1 = level k+1 prefetched into
  // registers, 2 = like 0, and the neighbour-level values (paph/pmfu/pmfd/plu of
  // k, k+1) re-read every level instead of carried (fewer live registers,
  // more L2 traffic)
  // 3 = the first-consumed inputs of level k+1 (EarlyIn) issued in the middle
  // of level k (the physics' mid hook), the rest at the top of level k+1;
  // 4 = all inputs of level k+1 issued in the middle of level k
  constexpr bool PFX = PF == 1, NBR = PF == 2, PFM = PF == 3, PFA = PF == 4;
  const KArgs<real, S>& A0 = *(const KArgs<real, S>*)ka;
  const int nproma = A0.nproma, klev = A0.klev;
  const size_t u1 = (size_t)b * nproma;                            // [nblocks][nproma]
  const size_t u2 = (size_t)b * klev * nproma;                     // [nblocks][klev][nproma]
  const size_t uh = (size_t)b * (klev + 1) * nproma;               // [nblocks][klev+1][nproma]
  const size_t u3 = (size_t)b * 5 * klev * nproma;                 // [nblocks][5][klev][nproma]

  ColConst<real> cc;
  Neighbors<real> nb;
  LevelIn<real> cur, nxt;
  EarlyIn<real> nxt_e;
  int ncldtop0;
  // F::spp: the column's own five parameters, formed here for every call -- a later KSEG segment sees what the first saw
  typename std::conditional<F::spp, SppCol<real, S, cptr<KArgs<real, S>>, LO>, NoSpp>::type spp;
  if constexpr (F::spp) { spp.ka = ka; spp.u1 = u1; spp.lane = lo0; }
  {
    CLOUDSC_PARAMS_HERE;
    const KArgs<real, S>& A = A0;
    ncldtop0 = c.ncldtop - 1;
    cc = column_constants(c, A, u1, uh, lo);
    if constexpr (F::spp) cc.kk_lcrit = cc.kk_lcrit * spp.mult(SPP_RCLCRIT);   // the column's own rclcrit_sea / rclcrit_land
    const int l1 = lev0 + 1 < klev ? lev0 + 1 : klev - 1;
    nb.paph_k = ldg(A.paph, uh + (size_t)lev0 * nproma, lo_half(lo));
    nb.paph_n = ldg(A.paph, uh + (size_t)(lev0 + 1) * nproma, lo_half(lo));
    nb.pmfu_k = ldg(A.pmfu, u2 + (size_t)lev0 * nproma, lo_full(lo));
    nb.pmfd_k = ldg(A.pmfd, u2 + (size_t)lev0 * nproma, lo_full(lo));
    nb.pmfu_n = ldg(A.pmfu, u2 + (size_t)l1 * nproma, lo_full(lo));
    nb.pmfd_n = ldg(A.pmfd, u2 + (size_t)l1 * nproma, lo_full(lo));
    nb.plu_n = ldg(A.plu, u2 + (size_t)l1 * nproma, lo_full(lo));
    if (PFX) load_level<real, AER, F::tb>(cur, A, u2, u3, lev0, klev, nproma, lo);
    if (PFM) load_early<real, F::tb>(nxt_e, A, u2, u3, lev0, klev, nproma, lo);
    if (PFA) load_level<real, AER, F::tb>(nxt, A, u2, u3, lev0, klev, nproma, lo);
  }
#if defined(__HIP_DEVICE_COMPILE__)
  // PF 1: drain the prologue's loads once (per segment) before the level loop.
  // The level-(k+1) prefetch at the top of each level first copies the previous
  // prefetch (cur = nxt); the waitcnt pass merges the loop header's two entries
  // (prologue, latch) conservatively and then made EVERY level wait for part of
  // the loads it had just issued -- a full memory round trip per level.  With
  // the prologue drained, the header needs no vmcnt wait: fp32 KSEG -3.7 %
  // (profiles/r03/experiment_prologue_drain_ab.txt).  (PF 3, the fp64 default,
  // measured neutral and keeps its schedule.)
  if constexpr (PFX) __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), expcnt(7), lgkmcnt(15)
#endif

  // fp32: the parameter block copied into VGPRs once per call (each value an
  // opaque per-lane copy), so the level loop reads every parameter from a
  // register instead of a scalar load + lgkmcnt(0) wait at each use -- 5 %
  // (profiles/r03/experiment_fp32_params_in_vgprs_ab.txt).  fp32 has the
  // registers for it (~95 VGPRs on top of ~155 at 2 waves/SIMD); fp64 would
  // need twice as many and keeps the scalar loads.
  constexpr bool PVR = sizeof(real) == 4;
  using PV = typename std::conditional<PVR, typename WithVgprParams<PT>::type, PT>::type;
  PV pv;
  if constexpr (PVR) {
    pv = *(const PV*)(const PT*)cpar;
    float* q = (float*)&pv;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(DevParams<float>) / sizeof(float)) - 4; i++) asm volatile("" : "+v"(q[i]));   // not the 4 ints
    if constexpr (F::spp)   // the raw parameters behind the ints, which only this form has
      for (int i = (int)(sizeof(DevParams<float>) / sizeof(float)); i < (int)(sizeof(PV) / sizeof(float)); i++)
        asm volatile("" : "+v"(q[i]));
  }
  for (int kloop = lev0; kloop < lev1; kloop++) {
    // the level index is laundered too, so no per-field induction pointers are formed
    int k = kloop;
    asm volatile("" : "+s"(k));
    // and so is the lane's 32-bit byte offset: its zero-extension is then formed
    // in this block, where the level loads fold it into the saddr + voffset form
    // instead of a 64-bit VGPR address add per load
    const LO lo = launder_vgpr(lo0);
    const bool physics = k >= ncldtop0;
    // ---- issue the loads of the next levels (software pipelining) ----
    real paph_nn, pmfu_nn, pmfd_nn, plu_nn;
    typename std::conditional<F::cml, CmlIn<real>, NoCml>::type cm;   // F::cml: this level's elements of BUFFER_CML
    {
      const KArgs<real, S>& A = *(const KArgs<real, S>*)launder_uniform(ka);
      // indices clamped instead of branched: the last levels re-read valid data
      const int k1 = k + 1 < klev ? k + 1 : klev - 1;
      const int k2 = k + 2 < klev ? k + 2 : klev - 1;
      const int kh2 = k + 2 < klev + 1 ? k + 2 : klev;
      if (!PFX && !PFM && !PFA) load_level<real, AER, F::tb>(cur, A, u2, u3, k, klev, nproma, lo);
      if (PFA) cur = nxt;
      if (PFM) {
        load_late<real, AER>(cur, A, u2, k, nproma, lo);
        take_early(cur, nxt_e);
      }
      if (PFX) load_level<real, AER, F::tb>(nxt, A, u2, u3, k1, klev, nproma, lo);
      if (NBR) {
        nb.paph_k = ldg(A.paph, uh + (size_t)k * nproma, lo_half(lo));
        nb.paph_n = ldg(A.paph, uh + (size_t)(k + 1) * nproma, lo_half(lo));
        const size_t i0 = u2 + (size_t)k * nproma, i1 = u2 + (size_t)k1 * nproma;
        nb.pmfu_k = ldg(A.pmfu, i0, lo_full(lo)); nb.pmfd_k = ldg(A.pmfd, i0, lo_full(lo));
        nb.pmfu_n = ldg(A.pmfu, i1, lo_full(lo)); nb.pmfd_n = ldg(A.pmfd, i1, lo_full(lo)); nb.plu_n = ldg(A.plu, i1, lo_full(lo));
        paph_nn = pmfu_nn = pmfd_nn = plu_nn = R(0.0);
      } else {
        // read once each (levels k+2 rotate through registers): streaming loads,
        // -0.4 % fp64 / -0.7 % fp32 against cached ones (profiles/r05/experiments_kernel_ab.txt)
        paph_nn = ldg1(A.paph, uh + (size_t)kh2 * nproma, lo_half(lo));
        const size_t i2 = u2 + (size_t)k2 * nproma;
        pmfu_nn = ldg1(A.pmfu, i2, lo_full(lo)); pmfd_nn = ldg1(A.pmfd, i2, lo_full(lo)); plu_nn = ldg1(A.plu, i2, lo_full(lo));
      }
      if constexpr (F::cml && CLOUDSC_CML_AT == 2) load_cml(cm, A, u2, k, klev, nproma, lo);
    }

    LevelState<real> ls;
    PhysOut<real> po;
    {
      const auto& c = params_here<PVR>(pv, cpar);
      init_level(c, cur, ls);
#pragma unroll
      for (int m = 0; m < 4; m++) { po.zqxn[m] = R(0.0); po.ctend[m] = R(0.0); }
      po.plude_k = cur.plude;
      po.atend = R(0.0);
      po.zcovptot_out = R(0.0);
      // PF 3: the next level's early inputs, issued in the middle of this level
      // (clamped at the last level: a re-read of valid data, never consumed)
      const auto mid = [&]() {
        if constexpr (F::cml && CLOUDSC_CML_AT == 1)
          load_cml(cm, *(const KArgs<real, S>*)launder_uniform(ka), u2, k, klev, nproma, launder_vgpr(lo0));
        if (PFM || PFA) {
          const int k1 = k + 1 < klev ? k + 1 : klev - 1;
          if (PFM)
            load_early<real, F::tb>(nxt_e, *(const KArgs<real, S>*)launder_uniform(ka), u2, u3, k1, klev, nproma,
                             launder_vgpr(lo0));
          else
            load_level<real, AER, F::tb>(nxt, *(const KArgs<real, S>*)launder_uniform(ka), u2, u3, k1, klev, nproma,
                                  launder_vgpr(lo0));
        }
      };
#ifndef CLOUDSC_ABLATE_PHYSICS   // timing-only diagnostic build: the level loop without sections 3-6
      if constexpr (F::spp) {
        if (physics) physics_level_spp(c, k, klev, ncldtop0, cur, nb, cc, ls, cs, po, mid, spp);
        else mid();
      } else {
        if (physics) physics_level(c, k, klev, ncldtop0, cur, nb, cc, ls, cs, po, mid);
        else mid();
      }
#else                            // (every load kept alive, so the bytes moved are the same)
      asm volatile("" :: "v"(cur.phrsw), "v"(cur.phrlw), "v"(cur.pvervel), "v"(cur.psnde), "v"(cur.psupsat),
                   "v"(nb.pmfu_k), "v"(nb.pmfd_k), "v"(nb.plu_n), "v"(cc.kk_pow));
      asm volatile("" :: "v"(cur.pclv[0]), "v"(cur.pclv[1]), "v"(cur.pclv[2]), "v"(cur.pclv[3]),
                   "v"(cur.ttcld[0]), "v"(cur.ttcld[1]), "v"(cur.ttcld[2]), "v"(cur.ttcld[3]));
      mid();
#endif
    }
    {
      const KArgs<real, S>& A = *(const KArgs<real, S>*)launder_uniform(ka);
      const auto& c = params_here<PVR>(pv, cpar);
      // (packed: a fresh copy as well, so that neither the top-of-level copy nor the
      // offsets formed from it stay live across the physics)
      const LO los = PVR || std::is_same<LO, PackLo>::value ? launder_vgpr(lo0) : lo;
      if constexpr (F::cml && CLOUDSC_CML_AT == 0) load_cml(cm, A, u2, k, klev, nproma, los);
      if constexpr (F::cml) store_level_cml(A, u2, k, klev, nproma, los, ls, po, cm);
      else if constexpr (F::adv) store_level_adv(c, A, u2, u3, k, klev, nproma, los, ls, po);
      else store_level<F::tb>(A, u2, u3, k, klev, nproma, los, physics, ls, po);
      flux_level<F::prog, F::surf>(c, A, uh + (size_t)(k + 1) * nproma, los, cur, ls, po, nb.paph_k, nb.paph_n, cs);
    }

    // ---- rotate carried state ----
    cs.t_prev = ls.ztp1; cs.a_prev = ls.za; cs.pap_prev = cur.pap;
    if (!NBR) {
      nb.paph_k = nb.paph_n; nb.paph_n = paph_nn;
      nb.pmfu_k = nb.pmfu_n; nb.pmfd_k = nb.pmfd_n;
      nb.pmfu_n = pmfu_nn; nb.pmfd_n = pmfd_nn; nb.plu_n = plu_nn;
    }
    if (PFX) cur = nxt;
  }
}

// carried state in registers (LDSC = false) or in LDS (LDSC = true)
template <typename real>
struct CarryRegs : CarryState<real> {
  __device__ __forceinline__ explicit CarryRegs(CLOUDSC_AS3 real*) {}
};
template <typename real, bool LDSC>
using CarryOf = typename std::conditional<LDSC, CarryLds<real>, CarryRegs<real>>::type;

// ===================== narrow blocks packed into full waves =====================
// NPROMA <= 32: one wave walks pack = 64 / nproma consecutive blocks b0 .. b0 +
// pack - 1 (a "group").  The memory layout is the reference's; each lane does
// exactly what the lane of the unpacked kernel serving its column does, so the
// output bits are the same.  The host passes this as an extra kernel argument
// (the unpacked kernels' arguments are untouched).
struct PackArgs {
  int pack;      // blocks per wave
  int nblocks;
  int ngroups;   // ceil(nblocks / pack)
};
// Lane l of the wave of group b0 / pack: sub-slot s = l / nproma, column jl = l %
// nproma of block b0 + s.  Returns whether the lane has a column: an inactive
// lane (l >= pack * nproma, a block or a column past the end) must issue no load
// and no store, its addresses may lie beyond the allocations.
template <typename S>
__device__ __forceinline__ bool pack_lane(int ngptot, int nproma, int klev, const PackArgs& G, int b0, PackLo& lo,
                                          unsigned& sub) {
  const unsigned l = threadIdx.x, np = (unsigned)nproma;
  const unsigned s = l / np, jl = l - s * np;
  lo.jb = jl * (unsigned)sizeof(S);
  lo.sb = s * np * (unsigned)sizeof(S);
  lo.klev = klev;
  sub = s;
  const unsigned b = (unsigned)b0 + s;                 // < nblocks + 64: no wrap
  // (b * np + jl is evaluated for every lane; where b < nblocks it is below
  // ngptot + nproma, where not its value is not used)
  return s < (unsigned)G.pack && b < (unsigned)G.nblocks && b * np + jl < (unsigned)ngptot;
}

// The one-shot kernel: a workgroup runs every level of its block (F::pack: one
// wave those of its group of G.pack blocks, b then the group's first block).
template <typename F>
__device__ __forceinline__ void cloudsc_kcache_body(cptr<typename F::fields> ka, cptr<typename F::params> cpar,
                                                    const PackArgs& G = PackArgs{1, 0, 0}) {
  using real = typename F::real;
  using S = typename F::store;
  using PT = typename F::params;
  const KArgs<real, S>& A = *(const KArgs<real, S>*)ka;
  const int b = F::pack ? (int)blockIdx.x * G.pack : (int)blockIdx.x;
  typename std::conditional<F::pack, PackLo, unsigned>::type lo;   // the lane's byte offset in a field plane
  if constexpr (F::pack) {
    unsigned sub;
    if (!pack_lane<S>(A.ngptot, A.nproma, A.klev, G, b, lo, sub)) return;
  } else {
    const int jl = threadIdx.x;
    if (jl >= A.nproma || b * A.nproma + jl >= A.ngptot) return;
    lo = (unsigned)jl * (unsigned)sizeof(S);
  }
  CarryOf<real, F::ldsc> cs(carry_lds_base<real>());
  init_carry<real, F::prog>(cs);
  {
    CLOUDSC_PARAMS_HERE;
    flux_top<F::prog, F::surf>(c, A, (size_t)b * (A.klev + 1) * A.nproma, lo);
  }
  kcache_levels<F>(ka, cpar, b, lo, 0, A.klev, cs);
  stg(((const KArgs<real, S>*)launder_uniform(ka))->prainfrac, (size_t)b * A.nproma, lo_surf(lane_here(lo)),
      cs.rainfrac);
  if constexpr (F::surf) {
    CLOUDSC_PARAMS_HERE;
    flux_surface(c, *(const KArgs<real, S>*)launder_uniform(ka), (size_t)b * A.nproma, lane_here(lo), cs);
  }
}

// ===================== persistent (work-queue) SCC-k-caching =====================
// Each column's level loop is cut into NSEG segments; an item is (segment s,
// block b), dequeued in order s-major from an atomic counter.  Segment s of
// block b waits for segment s-1 of b (flag[b] >= s) and resumes from the carried
// state it left in HBM ([nblocks][kCarryN][nproma], 19 values per column), so
// the result is bit-identical to the one-shot kernel.  Dequeue order guarantees
// progress: an item's predecessor was dequeued earlier by a running workgroup.
// The point: 2560 waves on 2048 wave slots leave the second round 75 % idle;
// with NSEG segments the tail shrinks to a fraction of a segment.
constexpr int kCarryN = 19;
constexpr int kMaxSeg = 16;
// Dequeue stripes (round 4): the items are split into kKsegStripes independent
// queues -- stripe s holds every segment of the blocks b with b % nstripes == s,
// in the same (segment, block, sub-block) order -- each with its own counter on
// its own 128-byte line, and workgroup w takes its items from stripe
// w % nstripes (the round-robin dispatch puts it on XCD w % 8).  At start-up
// 2048 workgroups then queue on 8 counters instead of one (round 3: the last
// first item began 23 us after the first).  Progress needs no residency: within
// a stripe items are dequeued in order, so an item's predecessor (the same
// block's previous segment, same stripe) was dequeued earlier by a running
// workgroup.  A stripe's counter advances by exactly its items plus the
// workgroups of the stripe per launch (each takes one ticket past the end).
constexpr int kKsegStripes = 8;
constexpr int kKsegCtrStride = 32;   // words between stripe counters (128 B)

#ifdef CLOUDSC_KSEG_TRACE
constexpr int kTraceMax = 1 << 16;
__device__ unsigned long long g_kseg_trace[4 * kTraceMax];
#endif

template <typename real>
struct PersistArgs {
  // The workspace is zeroed before the first launch on it; later launches on
  // the same workspace (a state's steps) need no zeroing: each launch takes
  // exactly nitems + grid tickets, so the host passes the counter's value at
  // its start (base), and flags are stamped per launch (stamp + segments done;
  // an older launch's flag compares as "not yet": signed difference).
  unsigned* ctr;          // stripe s's dequeue counter at ctr[s * kKsegCtrStride]: its tickets are
                          // base[s], base[s] + 1, ...
  unsigned* flags;        // [nblocks * nsub] stamp + segments completed
  unsigned* err;          // spin-limit violations (sticky until read, cloudsc_gpu_check)
  unsigned base[kKsegStripes];   // 0 right after zeroing
  unsigned stamp;         // 0 right after zeroing
  int nstripes;           // 1..kKsegStripes, <= grid
  real* state;            // [nblocks][kCarryN][nproma]
  int nseg, nitems, nblocks;
  int nsub;               // 64-column sub-blocks per NPROMA block (one wave each)
  int sb_major;           // item order (segment, sub-block, block) instead of (segment, block, sub-block)
  unsigned spin_limit;    // polls before a consumer gives up (and counts an error)
  // [0] += shader-clock cycles (s_memtime), [1] += 100 MHz real-time ticks
  // (s_memrealtime) each workgroup spends in the kernel: their ratio is the
  // effective shader clock of the launches (cloudsc_state_kseg_clock)
  unsigned long long* clk;
  int lev[kMaxSeg + 1];
};

// write-through (sc1) store of a handed-off value: an agent-scope relaxed atomic
// store lowers to global_store sc1, so the hand-off needs no L2 write-back
// (release fence) on the producer side (cdna_hip_programming.md G16, R1)
__device__ __forceinline__ void stg_sc1(double* ubase, size_t uidx, unsigned lane_bytes, double v) {
  __hip_atomic_store((unsigned long long*)((char*)(ubase + uidx) + lane_bytes), __double_as_longlong(v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void stg_sc1(float* ubase, size_t uidx, unsigned lane_bytes, float v) {
  __hip_atomic_store((unsigned*)((char*)(ubase + uidx) + lane_bytes), __float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// PROG: the six flux planes 13..18 of the workspace are neither stored nor reloaded (their places
// stay: one workspace serves launches of either form)
template <bool PROG = false, typename real, typename CS>
__device__ __forceinline__ void carry_io(real* st, size_t u, size_t plane, unsigned lo, CS& cs, bool save) {
#define CLOUDSC_CARRY_IO(q, m)                                                  \
  if (save) stg_sc1(st, u + (size_t)(q) * plane, lo, (real)cs.m);               \
  else cs.m = ldg((const real*)st, u + (size_t)(q) * plane, lo);
  CLOUDSC_CARRY_IO(0, t_prev) CLOUDSC_CARRY_IO(1, a_prev) CLOUDSC_CARRY_IO(2, pap_prev)
  CLOUDSC_CARRY_IO(3, zanewm1) CLOUDSC_CARRY_IO(4, zcovptot) CLOUDSC_CARRY_IO(5, zcovpmax)
  CLOUDSC_CARRY_IO(6, zcldtopdist) CLOUDSC_CARRY_IO(7, rainfrac) CLOUDSC_CARRY_IO(8, qxnm1_l)
  CLOUDSC_CARRY_IO(9, qxnm1_i) CLOUDSC_CARRY_IO(10, pfx_i) CLOUDSC_CARRY_IO(11, pfx_r)
  CLOUDSC_CARRY_IO(12, pfx_s)
  if constexpr (!PROG) {
    CLOUDSC_CARRY_IO(13, fl_lf) CLOUDSC_CARRY_IO(14, fl_if) CLOUDSC_CARRY_IO(15, fl_lng)
    CLOUDSC_CARRY_IO(16, fl_nng) CLOUDSC_CARRY_IO(17, fl_ltur) CLOUDSC_CARRY_IO(18, fl_itur)
  }
#undef CLOUDSC_CARRY_IO
}

// F::pack: the schedule runs over groups of G.pack blocks instead of blocks (items
// are (segment, group), stripes are taken over groups, one flag per group: the
// first G.ngroups words of the flag area); the carried state keeps its layout.
template <typename F>
__device__ __forceinline__ void cloudsc_kcache_persistent_body(cptr<typename F::fields> ka,
                                                               cptr<typename F::params> cpar,
                                                               const PersistArgs<typename F::real>& P,
                                                               const PackArgs& G = PackArgs{1, 0, 0}) {
  using real = typename F::real;
  using ST = typename F::store;
  using PT = typename F::params;
  constexpr bool PACK = F::pack;
  __shared__ int s_item;
  const KArgs<real, ST>& A = *(const KArgs<real, ST>*)ka;
  const int nproma = A.nproma, nsub = PACK ? 1 : P.nsub;
  // Every branch around a barrier is wave-uniform, and visibly so to the
  // compiler (SGPR conditions): the first wave of the workgroup does the
  // dequeue, the polling and the flag store with all of its lanes (same address,
  // same value), never a lane-0-only region.  A divergent `if (lane == 0)`
  // inside this loop gets restructured into nested exec-masked loops whose
  // barriers no longer pair up across waves.
  const bool wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x) < 64;
  const unsigned one = threadIdx.x == 0 ? 1u : 0u;  // lane 0 counts, the others add 0
  const unsigned long long clk0 = __builtin_amdgcn_s_memtime(), rt0 = __builtin_amdgcn_s_memrealtime();
  // this workgroup's stripe: blocks b = lb * S + st, lb < nbs (all wave-uniform)
  const int S = P.nstripes;
  const int st = (int)(blockIdx.x % (unsigned)S);
  const int nbs = ((PACK ? G.ngroups : P.nblocks) - st + S - 1) / S;
  const int nsbs = nbs * nsub;                        // items per segment in the stripe
  const int items = P.nseg * nsbs;
  unsigned* const ctr = P.ctr + st * kKsegCtrStride;
  const unsigned base = P.base[st];
  for (;;) {
    if (wave0) {
      const unsigned old = __hip_atomic_fetch_add(ctr, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_item = (int)(__builtin_amdgcn_readfirstlane(old) - base);   // lane 0's value: the ticket
    }
    __syncthreads();
    const int item = __builtin_amdgcn_readfirstlane(s_item);
    __syncthreads();                                   // s_item is rewritten next iteration
    if (item >= items) break;
    // item = (segment, stripe block lb, 64-column sub-block h), segment-major
    // (or (segment, h, lb) with sb_major): a block of NPROMA > 64 columns is run
    // as nsub one-wave items over the same block layout (sub-block h is the 64
    // contiguous columns h*64.. of each plane); flags are per (b, h)
    const int seg = item / nsbs, r = item - seg * nsbs;
    const int lb = P.sb_major ? r % nbs : r / nsub;
    const int hh = P.sb_major ? r / nbs : r - lb * nsub;
    const int ug = lb * S + st;                        // the block, or the group of blocks
    const int sb = ug * nsub + hh;
    const int b = PACK ? ug * G.pack : ug;             // packed: the group's first block
    const int jl = hh * 64 + (int)threadIdx.x;
    // the lane's byte offset in a field plane (storage type) and in a plane of
    // the carried state in the workspace (compute type): one value unless mixed
    typename std::conditional<PACK, PackLo, unsigned>::type lo;
    unsigned lo_c;
    bool active;
    if constexpr (PACK) {
      unsigned sub;
      active = pack_lane<ST>(A.ngptot, nproma, A.klev, G, b, lo, sub);
      lo = lane_here(lo);
      // sub-slot `sub` is a whole block of carried state ([kCarryN][nproma]) further on
      lo_c = (lo.sb * (unsigned)kCarryN + lo.jb) / (unsigned)sizeof(ST) * (unsigned)sizeof(real);
    } else {
      lo = (unsigned)jl * (unsigned)sizeof(ST);
      lo_c = (unsigned)jl * (unsigned)sizeof(real);
      active = jl < nproma && b * nproma + jl < A.ngptot;
    }
#ifdef CLOUDSC_KSEG_TRACE
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
    unsigned long long t_ready = t_start;
#endif
    const size_t ust = (size_t)b * kCarryN * nproma;
    CarryOf<real, F::ldsc> cs(carry_lds_base<real>());
    if (seg == 0) {
      init_carry<real, F::prog>(cs);
      if constexpr (!F::surf) {   // (the surface-fluxes form stores nothing at the top)
        if (active) {
          CLOUDSC_PARAMS_HERE;
          flux_top<F::prog, F::surf>(c, A, (size_t)b * (A.klev + 1) * nproma, lo);
        }
      }
    } else {
      // consumer: one relaxed poll (bounded, with s_sleep), one agent acquire,
      // wait, barrier, plain loads
      if (wave0) {
        for (unsigned spins = 0;; spins++) {
          if (spins >= P.spin_limit) {                   // bounded: never hang; the host reports it
            __hip_atomic_fetch_add(P.err, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
          }
          const unsigned f = __builtin_amdgcn_readfirstlane(
              __hip_atomic_load(P.flags + sb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          if ((int)(f - (P.stamp + (unsigned)seg)) >= 0) break;
          __builtin_amdgcn_s_sleep(4);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
#ifdef CLOUDSC_KSEG_TRACE
      t_ready = __builtin_amdgcn_s_memrealtime();
#endif
      if (active) carry_io<F::prog>(P.state, ust, (size_t)nproma, lo_c, cs, false);
    }
    if (active) kcache_levels<F>(ka, cpar, b, lo, P.lev[seg], P.lev[seg + 1], cs);
    const auto lo_e = lane_here(lo);   // packed: the offsets below formed here, not live across the levels
    if constexpr (PACK) lo_c = (lo_e.sb * (unsigned)kCarryN + lo_e.jb) / (unsigned)sizeof(ST) * (unsigned)sizeof(real);
    if (seg + 1 < P.nseg) {
      // producer (G16 R1): sc1 payload stores, every wave drains, barrier, the
      // flag stored with an agent atomic
      if (active) carry_io<F::prog>(P.state, ust, (size_t)nproma, lo_c, cs, true);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (wave0) __hip_atomic_store(P.flags + sb, P.stamp + (unsigned)(seg + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (active) {
      if constexpr (F::surf) {   // the last segment ends at the last level: the surface row of the four fluxes
        CLOUDSC_PARAMS_HERE;
        flux_surface(c, *(const KArgs<real, ST>*)launder_uniform(ka), (size_t)b * nproma, lo_e, cs);
      }
      stg(((const KArgs<real, ST>*)launder_uniform(ka))->prainfrac, (size_t)b * nproma, lo_surf(lo_e), cs.rainfrac);
    }
#ifdef CLOUDSC_KSEG_TRACE
    const int gitem = seg * P.nblocks * nsub + sb;   // the item's index in the unstriped order
    if (threadIdx.x == 0 && gitem < kTraceMax) {   // diagnostic build only: schedule of every item
      g_kseg_trace[4 * gitem + 0] = t_start;
      g_kseg_trace[4 * gitem + 1] = __builtin_amdgcn_s_memrealtime();
      g_kseg_trace[4 * gitem + 2] = blockIdx.x;
      g_kseg_trace[4 * gitem + 3] = t_ready;
    }
#endif
  }
  // the workgroup's time in the kernel, in shader cycles and real-time ticks
  // (one vector atomic each, after the last item; no barrier follows)
  const unsigned long long dclk = __builtin_amdgcn_s_memtime() - clk0, drt = __builtin_amdgcn_s_memrealtime() - rt0;
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(P.clk, dclk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(P.clk + 1, drt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace cloudsc
