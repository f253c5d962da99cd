// cloudsc_params.h -- the host-side folding of cloudsc_params_t into the
// kernels' DevParams<real> block (shared by the GPU launch path and the CPU
// variant).  Products and reciprocals the reference evaluates per point are
// computed once here with the SAME single IEEE operation, so results do not
// change (each member of DevParams cites the reference line it replaces).
// And the one place cloudsc_fields_t becomes the kernels' argument block: KArgs
// (cloudsc_kcache.h) keeps its own short names, read at fixed kernarg offsets,
// so that mapping is written by hand.
#pragma once
#include <cstring>

#include "cloudsc_amd.h"
#include "cloudsc_kcache.h"

namespace cloudsc {

template <typename real>
inline DevParamsSpp<real> fold_params(const cloudsc_params_t& p) {
  DevParamsSpp<real> d;
  std::memset(&d, 0, sizeof(d));
#define CP(n) d.n = (real)p.n
  CP(ptsphy); CP(rg); CP(rd); CP(retv); CP(rlvtt); CP(rlstt); CP(rtt); CP(rv);
  CP(r2es); CP(r3les); CP(r3ies); CP(r4les); CP(r4ies); CP(r5les); CP(r5ies); CP(r5alvcp); CP(r5alscp);
  CP(ralvdcp); CP(ralsdcp); CP(ralfdcp); CP(rtwat); CP(rtice); CP(rtwat_rtice_r); CP(rkoop1); CP(rkoop2);
  CP(ramid); CP(rprecrhmax); CP(rtaumel); CP(ramin); CP(rlmin); CP(rlcritsnow); CP(rsnowlin2);
  CP(riceinit); CP(rvice); CP(rvrain); CP(rvsnow); CP(rthomo); CP(rcovpmin); CP(rnice); CP(rcldtopcf);
  CP(rdepliqrefrate); CP(rdepliqrefdepth); CP(rvrfactor); CP(rclcrit_sea); CP(rclcrit_land);
  CP(rcl_kkaac); CP(rcl_kkbac); CP(rcl_kkaau); CP(rcl_kkbauq); CP(rcl_kkbaun); CP(rcl_kk_cloud_num_sea);
  CP(rcl_kk_cloud_num_land); CP(rcl_const1s); CP(rcl_const7s); CP(rcl_const8s); CP(rdensref);
  CP(rcl_cdenom1); CP(rcl_cdenom2); CP(rcl_cdenom3); CP(rcl_const1r); CP(rcl_const2r); CP(rcl_const3r);
  CP(rcl_const4r); CP(rcl_fac1); CP(rcl_fac2); CP(rcl_const5r); CP(rcl_const6r); CP(rcl_fzrab);
  // Host folding in the working precision: the same single IEEE operation the
  // reference evaluates per point (x86-64 host float/double arithmetic is IEEE).
  const real ptsphy = (real)p.ptsphy, rg = (real)p.rg, rd = (real)p.rd, rcpd = (real)p.rcpd;
  volatile real one = (real)1.0;   // keep the compiler from re-associating
  d.zqtmst = one / ptsphy;
  d.zrdcp = rd / rcpd;
  d.zrg_r = one / rg;
  d.zrldcp = one / ((real)p.ralsdcp - (real)p.ralvdcp);
  d.zinv_tsrg = one / (ptsphy * rg);
  d.half_rg = (real)0.5 * rg;
  d.zldifdt0 = (real)p.rcldiff * ptsphy;
  d.zldifdt_conv = (real)p.rcldiff_convi * d.zldifdt0;
  d.zfaci_koop = ptsphy / (real)p.rkooptau;
  d.zzco_snow = ptsphy * (real)p.rsnowlin1;
  d.rv_rd = (real)p.rv / rd;
  d.rg_rpecons = rg * (real)p.rpecons;
  d.one_m_ramin = one - (real)p.ramin;
  d.rd_rcp = one / rd;
  d.rtaumel_rcp = one / (real)p.rtaumel;
  d.rdepliqrefdepth_rcp = one / (real)p.rdepliqrefdepth;
  d.rvrfactor_rcp = one / (real)p.rvrfactor;
  d.nssopt = p.nssopt;
  d.ncldtop = p.ncldtop;
  d.laericesed = p.laericesed;
  d.laericeauto = p.laericeauto;
  CP(rcldiff); CP(rcldiff_convi); CP(rpecons);   // raw, for the per-column multiplier form
#undef CP
  return d;
}

// plude read in place (plude_in == plude); par: the launch's device parameter block, NULL for the host build
template <typename real, typename store = real>
KArgs<real, store> make_kargs(const cloudsc_fields_t* f, int ngptot, int nproma, int klev,
                              const DevParams<real>* par) {
  using in = const store*;
  using out = store*;
  KArgs<real, store> a{};
  a.pt = (in)f->pt; a.pq = (in)f->pq; a.ttt = (in)f->tendency_tmp_t; a.ttq = (in)f->tendency_tmp_q;
  a.tta = (in)f->tendency_tmp_a; a.ttcld = (in)f->tendency_tmp_cld; a.pvfl = (in)f->pvfl; a.pvfi = (in)f->pvfi;
  a.phrsw = (in)f->phrsw; a.phrlw = (in)f->phrlw; a.pvervel = (in)f->pvervel; a.pap = (in)f->pap;
  a.paph = (in)f->paph; a.plsm = (in)f->plsm; a.ktype = f->ktype; a.plu = (in)f->plu; a.psnde = (in)f->psnde;
  a.pmfu = (in)f->pmfu; a.pmfd = (in)f->pmfd; a.pa = (in)f->pa; a.pclv = (in)f->pclv; a.psupsat = (in)f->psupsat;
  a.picrit_aer = (in)f->picrit_aer; a.pre_ice = (in)f->pre_ice; a.pnice = (in)f->pnice;   // plcrit_aer, pccn: not read
  a.plude_in = (in)f->plude; a.plude = (out)f->plude; a.tlt = (out)f->tendency_loc_t; a.tlq = (out)f->tendency_loc_q;
  a.tla = (out)f->tendency_loc_a; a.tlcld = (out)f->tendency_loc_cld; a.pcovptot = (out)f->pcovptot;
  a.prainfrac = (out)f->prainfrac_toprfz; a.pfsqlf = (out)f->pfsqlf; a.pfsqif = (out)f->pfsqif;
  a.pfcqnng = (out)f->pfcqnng; a.pfcqlng = (out)f->pfcqlng; a.pfsqrf = (out)f->pfsqrf; a.pfsqsf = (out)f->pfsqsf;
  a.pfcqrng = (out)f->pfcqrng; a.pfcqsng = (out)f->pfcqsng; a.pfsqltur = (out)f->pfsqltur;
  a.pfsqitur = (out)f->pfsqitur; a.pfplsl = (out)f->pfplsl; a.pfplsn = (out)f->pfplsn; a.pfhpsl = (out)f->pfhpsl;
  a.pfhpsn = (out)f->pfhpsn;
  a.par = par; a.ngptot = ngptot; a.nproma = nproma; a.klev = klev;
  return a;
}

}  // namespace cloudsc
