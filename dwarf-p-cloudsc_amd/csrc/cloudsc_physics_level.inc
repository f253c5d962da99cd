// cloudsc_physics_level.inc -- the physics of one level, sections 3 to 6 (cloudsc_c.c:732-2508): the body of
// physics_level and, included a second time with CLOUDSC_PHYSICS_SPP 1, of physics_level_spp, the same physics
// with a column's own RAMID, RCLDIFF, RLCRITSNOW and RPECONS (SppCol, cloudsc_kcache.h).  One text, switched by
// the preprocessor and not by `if constexpr`: physics_level then compiles from exactly the tokens it had before
// the per-column multiplier form existed, which is what keeps every other kernel's register allocation where it
// was (DESIGN.md 3.28: one more by-reference argument of the shared body moved eight fp32 kernels).
// Included by cloudsc_kcache.h only, inside namespace cloudsc.
#if CLOUDSC_PHYSICS_SPP
template <typename real, typename P, typename CS, typename Mid, typename SP>
CLOUDSC_HD void physics_level_spp(const P& c, const int k, const int klev,
                                                  const int ncldtop0, const LevelIn<real>& in,
                                                  const Neighbors<real>& nb, const ColConst<real>& cc,
                                                  LevelState<real>& ls, CS& cs, PhysOut<real>& po,
                                                  const Mid& mid, const SP& spp) {
#else
template <typename real, typename P, typename CS, typename Mid = NoMidHook>
CLOUDSC_HD void physics_level(const P& c, const int k, const int klev,
                                              const int ncldtop0, const LevelIn<real>& in,
                                              const Neighbors<real>& nb, const ColConst<real>& cc,
                                              LevelState<real>& ls, CS& cs, PhysOut<real>& po,
                                              const Mid& mid = Mid{}) {
#endif
  const real zepsilon = R(100.0) * (sizeof(real) == 8 ? (real)__DBL_EPSILON__ : (real)__FLT_EPSILON__);
  const real zepsec = R(1.0e-14);
  const real ztw1 = R(1329.31000000000), ztw2 = R(0.00746150000000000), ztw3 = R(85000.0000000000);
  const real ztw4 = R(40.6370000000000), ztw5 = R(275.000000000000);
  const real ztp1 = ls.ztp1, za = ls.za, zaorig = ls.zaorig, zfoealfa = ls.zfoealfa;
  const real* zqx = ls.zqx;
  const real* zqx0 = ls.zqx0;
  real& ttend = ls.ttend;
  real& qtend = ls.qtend;
  real* zqxn = po.zqxn;
  real* ctend = po.ctend;
  real& plude_k = po.plude_k;
  real& atend = po.atend;

    const real pap_k = in.pap;
    // saturation values (:583-609)
    real e_liq, e_ice;
    if (CLOUDSC_RUN(AB_SAT)) {
      exp_liq_ice<real>(c, ztp1, e_liq, e_ice);
    } else {
      e_liq = launder_vgpr(ztp1 * R(0.02));
      e_ice = launder_vgpr(ztp1 * R(0.019));
    }
    // divisors shared by several divisions (cl_recip: one reciprocal, same quotient bits)
    const Recip<real> r_pap = cl_recip_p<real>(c, pap_k);
    const real zfoeewmt = fmin(cl_div_p<real>(c, (c.r2es * (zfoealfa * e_liq + (R(1.0) - zfoealfa) * e_ice)), r_pap), R(0.5));
    const Recip<real> r_mixd = cl_recip_p<real>(c, R(1.0) - c.retv * zfoeewmt);
    const real zqsmix = cl_div_p<real>(c, zfoeewmt, r_mixd);
    const real zalfa_d = fmax(R(0.0), copysign(R(1.0), ztp1 - c.rtt));
    real zfoeew = fmin(cl_div_p<real>(c, (zalfa_d * (c.r2es * e_liq) + (R(1.0) - zalfa_d) * (c.r2es * e_ice)), r_pap), R(0.5));
    zfoeew = fmin(R(0.5), zfoeew);
    const Recip<real> r_iced = cl_recip_p<real>(c, R(1.0) - c.retv * zfoeew);
    const real zqsice = cl_div_p<real>(c, zfoeew, r_iced);
    // (zqsliq, :601-604, is computed where rain evaporation, its only reader, runs)
    // liquid/ice fractions (:628-636)
    const real zli = zqx[QL] + zqx[QI];
    real zliqfrac = R(0.0), zicefrac = R(0.0);
    if (zli > c.rlmin) {
      zliqfrac = cl_div_p<real>(c, zqx[QL], zli);
      zicefrac = R(1.0) - zliqfrac;
    }

    // ===== 3. physics (:732-2508) =====
    real zqxfg[5];
  #pragma unroll
    for (int m = 0; m < 5; m++) zqxfg[m] = zqx[m];
    // zsolqa is dense in the reference; only 13 entries can become non-zero
    // here, kept as named scalars sa_<a><b> == zsolqa[a][b] (C indexing).  Every
    // off-diagonal pair is updated antisymmetrically (x to one, -x to the other,
    // in the same order, and scaled by the same factors in 5.2), and IEEE
    // negation is exact and sign-symmetric under round-to-nearest, so
    // zsolqa[b][a] == -zsolqa[a][b] exactly: only one of each pair is stored.
    //   stored: ll ii rr ss (diagonal)  lv iv li ls lr ir sr rv sv
    //   implied: vl=-lv vi=-iv il=-li sl=-ls rl=-lr ri=-ir rs=-sr vr=-rv vs=-sv
    real sa_ll = 0, sa_ii = 0, sa_rr = 0, sa_ss = 0;
    real sa_lv = 0, sa_iv = 0, sa_li = 0, sa_ls = 0, sa_lr = 0, sa_ir = 0, sa_sr = 0, sa_rv = 0, sa_sv = 0;
    // zsolqb non-zeros: [ql][ql], [qi][qi] (subsidence), [qi][qs] (snow autoconv), [ql][qs] (riming)
    real sb_ll = 0, sb_ii = 0, sb_is = 0, sb_ls = 0;
    real conv_src_l = 0, conv_src_i = 0, conv_sink = 0, psup_l = 0, psup_i = 0;
    real fsrc_i = 0, fsrc_r = 0, fsrc_s = 0;
    real zqpretot = R(0.0), zsolab = R(0.0), zsolac = R(0.0);

    // 3.0 derived variables (:799-841)
    const real zdp = nb.paph_n - nb.paph_k;
    const real zgdp = cl_div_p<real>(c, c.rg, zdp);
    const real zrho = cl_div_p<real>(c, pap_k, (c.rd * ztp1));
    const real zdtgdp = c.ptsphy * zgdp;
    const real zrdtgdp = zdp * c.zinv_tsrg;
    real zfacw, zfaci, zfac, zcor;
    { const real d = ztp1 - c.r4les; zfacw = cl_div_p<real>(c, c.r5les, (d * d)); }
    { const real d = ztp1 - c.r4ies; zfaci = cl_div_p<real>(c, c.r5ies, (d * d)); }
    zcor = cl_div_p<real>(c, R(1.0), r_iced);
    const real zdqsicedt = (zfaci * zcor) * zqsice;
    const real zcorqsice = R(1.0) + c.ralsdcp * zdqsicedt;
    zfac = zfoealfa * zfacw + (R(1.0) - zfoealfa) * zfaci;
    zcor = cl_div_p<real>(c, R(1.0), r_mixd);
    const real zdqsmixdt = (zfac * zcor) * zqsmix;
    const real zcorqsmix = R(1.0) + (zfoealfa * c.ralvdcp + (R(1.0) - zfoealfa) * c.ralsdcp) * zdqsmixdt;
    const real zevaplimmix = fmax(cl_div_p<real>(c, (zqsmix - zqx[QV]), zcorqsmix), R(0.0));
    real ztmpa = cl_div_p<real>(c, R(1.0), fmax(za, zepsec));
    const Recip<real> r_1mza = cl_recip_p<real>(c, fmax(zepsec, R(1.0) - za));
    real zliqcld = zqx[QL] * ztmpa;
    real zicecld = zqx[QI] * ztmpa;
    real zlicld = zliqcld + zicecld;

    // evaporate very small amounts of liquid and ice (:846-859)
    if (zqx[QL] < c.rlmin) { sa_lv = zqx[QL]; }
    if (zqx[QI] < c.rlmin) { sa_iv = zqx[QI]; }

    // 3.1 ice supersaturation adjustment (:874-954)
    const real zfokoop = fmin(c.rkoop1 - c.rkoop2 * ztp1, cl_div_p<real>(c, (c.r2es * e_liq) * R(1.0), (c.r2es * e_ice)));
    if (c.nssopt == 0 || ztp1 >= c.rtt) {
      zfac = R(1.0);
      zfaci = R(1.0);
    } else {
      zfac = za + zfokoop * (R(1.0) - za);
      zfaci = c.zfaci_koop;
    }
    real zsupsat = R(0.0);
    if (!CLOUDSC_RUN(AB_SUPSAT)) {
    } else if (za > c.one_m_ramin) {
      zsupsat = fmax(cl_div_p<real>(c, (zqx[QV] - zfac * zqsice), zcorqsice), R(0.0));
    } else {
      const real zqp1env = cl_div_p<real>(c, (zqx[QV] - za * zqsice), fmax(R(1.0) - za, zepsilon));
      zsupsat = fmax(cl_div_p<real>(c, ((R(1.0) - za) * (zqp1env - zfac * zqsice)), zcorqsice), R(0.0));
    }
    const bool warm_homo = ztp1 > c.rthomo;
    if (zsupsat > zepsec) {
      if (warm_homo) { sa_lv = sa_lv - zsupsat; zqxfg[QL] = zqxfg[QL] + zsupsat;
      } else { sa_iv = sa_iv - zsupsat; zqxfg[QI] = zqxfg[QI] + zsupsat;
      }
      zsolac = (R(1.0) - za) * zfaci;
    }
    if (CLOUDSC_RUN(AB_SUPSAT) && in.psupsat > zepsec) {
      if (warm_homo) {
        sa_ll = sa_ll + in.psupsat; psup_l = in.psupsat; zqxfg[QL] = zqxfg[QL] + in.psupsat;
      } else {
        sa_ii = sa_ii + in.psupsat; psup_i = in.psupsat; zqxfg[QI] = zqxfg[QI] + in.psupsat;
      }
      zsolac = (R(1.0) - za) * zfaci;
    }

    // 3.2 detrainment from convection (:967-987)
    if (CLOUDSC_RUN(AB_CONV) && k < klev - 1) {
      plude_k = plude_k * zdtgdp;
      if (nb.plu_n > zepsec && plude_k > c.rlmin) {
        zsolac = zsolac + cl_div_p<real>(c, plude_k, nb.plu_n);
        conv_src_l = zfoealfa * plude_k;
        conv_src_i = (R(1.0) - zfoealfa) * plude_k;
        sa_ll = sa_ll + conv_src_l;
        sa_ii = sa_ii + conv_src_i;
      } else {
        plude_k = R(0.0);
      }
      sa_ss = sa_ss + in.psnde * zdtgdp;
    }

    // 3.3 subsidence source from the layer above + evaporation (:1002-1058)
    if (CLOUDSC_RUN(AB_CONV) && k > ncldtop0) {
      const real zmf = fmax(R(0.0), (nb.pmfu_k + nb.pmfd_k) * zdtgdp);
      real zacust = zmf * cs.zanewm1;
      const real zlcust_l = zmf * cs.qxnm1_l;
      const real zlcust_i = zmf * cs.qxnm1_i;
      conv_src_l = conv_src_l + zlcust_l;
      conv_src_i = conv_src_i + zlcust_i;
      const real zdtdp = cl_div_p<real>(c, ((c.zrdcp * R(0.5)) * (cs.t_prev + ztp1)), nb.paph_k);
      const real zdtforc = zdtdp * (pap_k - cs.pap_prev);
      const real zdqs = (cs.zanewm1 * zdtforc) * zdqsmixdt;
      real zlfinalsum = R(0.0);
      {
        real zlfinal = fmax(R(0.0), zlcust_l - zdqs);
        const real zevap = fmin(zlcust_l - zlfinal, zevaplimmix);
        zlfinal = zlcust_l - zevap;
        zlfinalsum = zlfinalsum + zlfinal;
        sa_ll = sa_ll + zlcust_l; sa_lv = sa_lv + zevap;
      }
      {
        real zlfinal = fmax(R(0.0), zlcust_i - zdqs);
        const real zevap = fmin(zlcust_i - zlfinal, zevaplimmix);
        zlfinal = zlcust_i - zevap;
        zlfinalsum = zlfinalsum + zlfinal;
        sa_ii = sa_ii + zlcust_i; sa_iv = sa_iv + zevap;
      }
      if (zlfinalsum < zepsec) zacust = R(0.0);
      zsolac = zsolac + zacust;
    }

    // subsidence sink of cloud to the layer below (:1064-1075)
    if (CLOUDSC_RUN(AB_CONV) && k < klev - 1) {
      const real zmfdn = fmax(R(0.0), (nb.pmfu_n + nb.pmfd_n) * zdtgdp);
      zsolab = zsolab + zmfdn;
      sb_ll = sb_ll + zmfdn;
      sb_ii = sb_ii + zmfdn;
      conv_sink = zmfdn;
    }

    // 3.4 erosion of clouds by turbulent mixing (:1087-1118)
#if CLOUDSC_PHYSICS_SPP
    // the column's own rcldiff: fold_params' operations, per lane
    const real spp_zldifdt0 = spp.zldifdt0(c);
    const real spp_zldifdt_conv = c.rcldiff_convi * spp_zldifdt0;
    const real zldifdt = (cc.ktype > 0 && plude_k > zepsec) ? spp_zldifdt_conv : spp_zldifdt0;
#else
    const real zldifdt = (cc.ktype > 0 && plude_k > zepsec) ? pval(c, c.zldifdt_conv) : pval(c, c.zldifdt0);
#endif
    if (CLOUDSC_RUN(AB_EROSION) && zli > zepsec) {
      const real ze = zldifdt * fmax(zqsmix - zqx[QV], R(0.0));
      real zleros = za * ze;
      zleros = fmin(zleros, zevaplimmix);
      zleros = fmin(zleros, zli);
      const real zaeros = cl_div_p<real>(c, zleros, zlicld);
      zsolac = zsolac - zaeros;
      sa_lv = sa_lv + zliqfrac * zleros;
      sa_iv = sa_iv + zicefrac * zleros;
    }

    CLOUDSC_MID_HOOK(1);
    // 3.4 condensation/evaporation due to dqsat/dt: two Newton steps (:1137-1182)
    real zdqs;
    if (!CLOUDSC_RUN(AB_NEWTON)) {
      zdqs = launder_vgpr((zqsmix - zqx[QV]) * R(0.1));   // stand-in of the right sign
    } else {
      const real zdtdp = cl_div_p<real>(c, (c.zrdcp * ztp1), r_pap);
      const real zdpmxdt = zdp * c.zqtmst;
      const real zmfdn = (k < klev - 1) ? nb.pmfu_n + nb.pmfd_n : R(0.0);
      real zwtot = in.pvervel + c.half_rg * (nb.pmfu_k + nb.pmfd_k + zmfdn);
      zwtot = fmin(zdpmxdt, fmax(-zdpmxdt, zwtot));
      const real zzzdt = in.phrsw + in.phrlw;
      const real zdtdiab = fmin(zdpmxdt * zdtdp, fmax(-zdpmxdt * zdtdp, zzzdt)) * c.ptsphy + c.ralfdcp * R(0.0);
      const real zdtforc = (zdtdp * zwtot) * c.ptsphy + zdtdiab;
      real tt = fmax(ztp1 + zdtforc, R(160.0));
      real qsm = zqsmix;
      const real zqp = cl_div_p<real>(c, R(1.0), r_pap);
  #pragma unroll
      for (int it = 0; it < 2; it++) {
        const real a = foealfa<real>(c, tt);
        real el, ei;
        exp_liq_ice<real>(c, tt, el, ei);
        real zqsat = (c.r2es * (a * el + (R(1.0) - a) * ei)) * zqp;
        zqsat = fmin(R(0.5), zqsat);
        const real zcor2 = cl_div_p<real>(c, R(1.0), (R(1.0) - c.retv * zqsat));
        zqsat = zqsat * zcor2;
        const real zcond = cl_div_p<real>(c, (qsm - zqsat), (R(1.0) + (zqsat * zcor2) * foedem_term<real>(c, tt, a)));
        tt = tt + (a * c.ralvdcp + (R(1.0) - a) * c.ralsdcp) * zcond;
        qsm = qsm - zcond;
      }
      zdqs = qsm - zqsmix;
    }

    // 3.4a evaporation of clouds (:1189-1207)
    if (CLOUDSC_RUN(AB_COND) && zdqs > R(0.0)) {
      real zlevap = za * fmin(zdqs, zlicld);
      zlevap = fmin(zlevap, zevaplimmix);
      zlevap = fmin(zlevap, fmax(zqsmix - zqx[QV], R(0.0)));
      sa_lv = sa_lv + zliqfrac * zlevap;
      sa_iv = sa_iv + zicefrac * zlevap;
    }
    // 3.4b(1) increase of cloud water in existing clouds (:1213-1250)
    if (CLOUDSC_RUN(AB_COND) && zdqs <= -c.rlmin && za > zepsec) {
      real zlcond1 = fmax(-zdqs, R(0.0));
      real zcdmax;
      if (za > R(0.99)) {
        const real zcor3 = cl_div_p<real>(c, R(1.0), (R(1.0) - c.retv * zqsmix));
        zcdmax = cl_div_p<real>(c, (zqx[QV] - zqsmix), (R(1.0) + (zcor3 * zqsmix) * foedem_term<real>(c, ztp1, zfoealfa)));
      } else {
        zcdmax = cl_div_p<real>(c, (zqx[QV] - za * zqsmix), za);
      }
      zlcond1 = fmax(fmin(zlcond1, zcdmax), R(0.0));
      zlcond1 = za * zlcond1;
      if (zlcond1 < c.rlmin) zlcond1 = R(0.0);
      if (warm_homo) { sa_lv = sa_lv - zlcond1; zqxfg[QL] = zqxfg[QL] + zlcond1;
      } else { sa_iv = sa_iv - zlcond1; zqxfg[QI] = zqxfg[QI] + zlcond1;
      }
    }
    // 3.4b(2) generation of new clouds (:1253-1363)
#if CLOUDSC_PHYSICS_SPP
    const real spp_ramid = spp.ramid(c);   // the column's own ramid, read ahead of the branch that uses it
    if (CLOUDSC_RUN(AB_COND) && zdqs <= -c.rlmin && za < R(1.0) - zepsec) {
      real zrhc = spp_ramid;
      const real zsigk = cl_div_p<real>(c, pap_k, cc.paph_sfc);
      if (zsigk > R(0.8)) {
        const real s = cl_div_lit_p<real>(c, (zsigk - R(0.8)), R(0.2));
        zrhc = spp_ramid + (R(1.0) - spp_ramid) * (s * s);
      }
#else
    if (CLOUDSC_RUN(AB_COND) && zdqs <= -c.rlmin && za < R(1.0) - zepsec) {
      real zrhc = c.ramid;
      const real zsigk = cl_div_p<real>(c, pap_k, cc.paph_sfc);
      if (zsigk > R(0.8)) {
        const real s = cl_div_lit_p<real>(c, (zsigk - R(0.8)), R(0.2));
        zrhc = c.ramid + (R(1.0) - c.ramid) * (s * s);
      }
#endif
      real zqe = R(0.0);
      if (c.nssopt == 0 || c.nssopt == 1) {
        zqe = cl_div_p<real>(c, (zqx[QV] - za * zqsice), r_1mza);
        zqe = fmax(R(0.0), zqe);
      } else if (c.nssopt == 2) {
        zqe = zqx[QV];
      } else if (c.nssopt == 3) {
        zqe = zqx[QV] + zli;
      }
      const real zfacn = (c.nssopt == 0 || ztp1 >= c.rtt) ? R(1.0) : zfokoop;
      if (zqe >= zqsice * zfacn * zrhc && zqe < zqsice * zfacn) {
        real zacond = cl_div_p<real>(c, -((R(1.0) - za) * zfacn) * zdqs, fmax(R(2.0) * (zfacn * zqsice - zqe), zepsec));
        zacond = fmin(zacond, R(1.0) - za);
        real zlcond2 = -(zfacn * zdqs) * R(0.5) * zacond;
        const real zzdl = cl_div_p<real>(c, (R(2.0) * (zfacn * zqsice - zqe)), fmax(zepsec, R(1.0) - za));
        if (zdqs * zfacn < -zzdl) {
          const real zlcondlim = ((za - R(1.0)) * zfacn) * zdqs - zfacn * zqsice + zqx[QV];
          zlcond2 = fmin(zlcond2, zlcondlim);
        }
        zlcond2 = fmax(zlcond2, R(0.0));
        if (R(1.0) - za < zepsec || zlcond2 < c.rlmin) {
          zlcond2 = R(0.0);
          zacond = R(0.0);
        }
        if (zlcond2 == R(0.0)) zacond = R(0.0);
        zsolac = zsolac + zacond;
        if (warm_homo) { sa_lv = sa_lv - zlcond2; zqxfg[QL] = zqxfg[QL] + zlcond2;
        } else { sa_iv = sa_iv - zlcond2; zqxfg[QI] = zqxfg[QI] + zlcond2;
        }
      }
    }

    CLOUDSC_MID_HOOK(2);
    // 3.7 growth of ice by vapour deposition, Rotstayn (:1382-1447)
    if (za >= c.rcldtopcf && cs.a_prev < c.rcldtopcf) cs.zcldtopdist = R(0.0);
    else cs.zcldtopdist = cs.zcldtopdist + cl_div_p<real>(c, zdp, (zrho * c.rg));
    if (CLOUDSC_RUN(AB_DEPOS) && zqxfg[QL] > c.rlmin && ztp1 < c.rtt) {
      const real zvpice = cl_div_known_p<real>(c, ((c.r2es * e_ice) * c.rv), c.rd, c.rd_rcp);
      const real zvpliq = zvpice * zfokoop;
      const real zicenuclei = R(1000.0) * cl_exp<real>(c, cl_div_p<real>(c, (R(12.96) * (zvpliq - zvpice)), zvpliq) - R(0.639));
      const real zadd = cl_div_p<real>(c, (c.rlstt * (cl_div_p<real>(c, c.rlstt, (c.rv * ztp1)) - R(1.0))), (R(0.024) * ztp1));
      const real zbdd = cl_div_p<real>(c, ((c.rv * ztp1) * pap_k), (R(2.21) * zvpice));
      const real zcvds = cl_div_p<real>(c, ((R(7.8) * cl_pow<real>(c, cl_div_p<real>(c, zicenuclei, zrho), R(0.666))) * (zvpliq - zvpice)), ((R(8.87) * (zadd + zbdd)) * zvpice));
      const real zice0 = fmax(zicecld, cl_div_p<real>(c, (zicenuclei * c.riceinit), zrho));
      const real zinew = cl_pow<real>(c, (R(0.666) * zcvds) * c.ptsphy + cl_pow<real>(c, zice0, R(0.666)), R(1.5));
      real zdepos = fmax(za * (zinew - zice0), R(0.0));
      zdepos = fmin(zdepos, zqxfg[QL]);
      const real zinfactor = fmin(cl_div_lit_p<real>(c, zicenuclei, R(15000.0)), R(1.0));
      zdepos = zdepos * fmin(zinfactor + (R(1.0) - zinfactor) * (c.rdepliqrefrate + cl_div_known_p<real>(c, cs.zcldtopdist, c.rdepliqrefdepth, c.rdepliqrefdepth_rcp)), R(1.0));
      sa_li = sa_li + zdepos;
      zqxfg[QI] = zqxfg[QI] + zdepos; zqxfg[QL] = zqxfg[QL] - zdepos;
    }

    // 4. revise in-cloud condensate (:1528-1533)
    ztmpa = cl_div_p<real>(c, R(1.0), fmax(za, zepsec));
    zliqcld = zqxfg[QL] * ztmpa;
    zicecld = zqxfg[QI] * ztmpa;
    zlicld = zliqcld + zicecld;

    CLOUDSC_MID_HOOK(3);
    // 4.2 sedimentation of ice, rain, snow (:1541-1576)
    if (CLOUDSC_RUN(AB_SEDIM) && k > ncldtop0) {
      fsrc_i = cs.pfx_i * zdtgdp; sa_ii = sa_ii + fsrc_i; zqxfg[QI] = zqxfg[QI] + fsrc_i; zqpretot = zqpretot + zqxfg[QI];
      fsrc_r = cs.pfx_r * zdtgdp; sa_rr = sa_rr + fsrc_r; zqxfg[QR] = zqxfg[QR] + fsrc_r; zqpretot = zqpretot + zqxfg[QR];
      fsrc_s = cs.pfx_s * zdtgdp; sa_ss = sa_ss + fsrc_s; zqxfg[QS] = zqxfg[QS] + fsrc_s; zqpretot = zqpretot + zqxfg[QS];
    }
    const real vqx_i = c.laericesed ? R(0.002) * in.pre_ice : pval(c, c.rvice);
    const real fsink_i = zdtgdp * (vqx_i * zrho);
    const real fsink_r = zdtgdp * (c.rvrain * zrho);
    const real fsink_s = zdtgdp * (c.rvsnow * zrho);

    // precip cover overlap, MAX-RAN (:1594-1611)
    real zcovpclr, zraincld, zsnowcld;
    if (CLOUDSC_RUN(AB_SEDIM) && zqpretot > zepsec) {
      cs.zcovptot = R(1.0) - cl_div_p<real>(c, (R(1.0) - cs.zcovptot) * (R(1.0) - fmax(za, cs.a_prev)), (R(1.0) - fmin(cs.a_prev, R(1.0) - R(1.0e-6))));
      cs.zcovptot = fmax(cs.zcovptot, c.rcovpmin);
      zcovpclr = fmax(R(0.0), cs.zcovptot - za);
      zraincld = cl_div_p<real>(c, zqxfg[QR], cs.zcovptot);
      zsnowcld = cl_div_p<real>(c, zqxfg[QS], cs.zcovptot);
      cs.zcovpmax = fmax(cs.zcovptot, cs.zcovpmax);
    } else {
      zraincld = R(0.0); zsnowcld = R(0.0); cs.zcovptot = R(0.0); zcovpclr = R(0.0); cs.zcovpmax = R(0.0);
    }

    const bool cold = ztp1 <= c.rtt;
    // 4.3a autoconversion to snow (:1616-1637)
#if CLOUDSC_PHYSICS_SPP
    const real spp_lcrit = spp.rlcritsnow(c);   // (not read under LAERICEAUTO)
    if (CLOUDSC_RUN(AB_AUTO) && cold && zicecld > zepsec) {
      real zzco = c.zzco_snow * cl_exp<real>(c, c.rsnowlin2 * (ztp1 - c.rtt));
      real zlcrit = spp_lcrit;
#else
    if (CLOUDSC_RUN(AB_AUTO) && cold && zicecld > zepsec) {
      real zzco = c.zzco_snow * cl_exp<real>(c, c.rsnowlin2 * (ztp1 - c.rtt));
      real zlcrit = pval(c, c.rlcritsnow);
#endif
      if (c.laericeauto) {
        zlcrit = in.picrit_aer;
        zzco = zzco * cl_pow<real>(c, cl_div_p<real>(c, c.rnice, in.pnice), R(0.333));
      }
      const real r = cl_div_p<real>(c, zicecld, zlcrit);
      sb_is = sb_is + zzco * (R(1.0) - cl_exp<real>(c, -(r * r)));
    }
    // 4.3b warm rain, Khairoutdinov and Kogan 2000 (:1644-1761)
    if (CLOUDSC_RUN(AB_AUTO) && zliqcld > zepsec) {
      real zrainaut = R(0.0), zrainacc = R(0.0);
      if (zliqcld > cc.kk_lcrit) {
        zrainaut = ((((R(1.5) * za) * c.ptsphy) * c.rcl_kkaau) * cl_pow<real>(c, zliqcld, c.rcl_kkbauq)) * cc.kk_pow;
        zrainaut = fmin(zrainaut, zqxfg[QL]);
        if (zrainaut < zepsec) zrainaut = R(0.0);
        zrainacc = (((R(2.0) * za) * c.ptsphy) * c.rcl_kkaac) * cl_pow<real>(c, zliqcld * zraincld, c.rcl_kkbac);
        zrainacc = fmin(zrainacc, zqxfg[QL]);
        if (zrainacc < zepsec) zrainacc = R(0.0);
      }
      if (cold) {
        sa_ls = sa_ls + zrainaut; sa_ls = sa_ls + zrainacc;
      } else {
        sa_lr = sa_lr + zrainaut; sa_lr = sa_lr + zrainacc;
      }
    }
    // riming of snow by cloud water (:1768-1808)
    if (CLOUDSC_RUN(AB_AUTO) && cold && zliqcld > zepsec && cs.zcovptot > R(0.01) && zsnowcld > zepsec) {
      const real zfallcorr = cl_pow<real>(c, cl_div_p<real>(c, c.rdensref, zrho), R(0.4));
      real zsnowrime = ((((R(0.3) * cs.zcovptot) * c.ptsphy) * c.rcl_const7s) * zfallcorr) *
                       cl_pow<real>(c, (zrho * zsnowcld) * c.rcl_const1s, c.rcl_const8s);
      zsnowrime = fmin(zsnowrime, R(1.0));
      sb_ls = sb_ls + zsnowrime;
    }

    CLOUDSC_MID_HOOK(4);
    // 4.4a melting of snow and ice (:1817-1859)
    const real zicetot = zqxfg[QI] + zqxfg[QS];
    if (CLOUDSC_RUN(AB_MELT) && zicetot > zepsec && ztp1 > c.rtt) {
      const real zsubsat = fmax(zqsice - zqx[QV], R(0.0));
      const real ztdmtw0 = ztp1 - c.rtt - zsubsat * (ztw1 + ztw2 * (pap_k - ztw3) - ztw4 * (ztp1 - ztw5));
      const real zcons1 = fabs(cl_div_known_p<real>(c, (c.ptsphy * (R(1.0) + R(0.5) * ztdmtw0)), c.rtaumel, c.rtaumel_rcp));
      const real zmeltmax = fmax((ztdmtw0 * zcons1) * c.zrldcp, R(0.0));
      if (zmeltmax > zepsec) {
        {   // ice -> rain
          const real zalfa = cl_div_p<real>(c, zqxfg[QI], zicetot);
          const real zmelt = fmin(zqxfg[QI], zalfa * zmeltmax);
          zqxfg[QI] = zqxfg[QI] - zmelt; zqxfg[QR] = zqxfg[QR] + zmelt;
          sa_ir = sa_ir + zmelt;
        }
        {   // snow -> rain
          const real zalfa = cl_div_p<real>(c, zqxfg[QS], zicetot);
          const real zmelt = fmin(zqxfg[QS], zalfa * zmeltmax);
          zqxfg[QS] = zqxfg[QS] - zmelt; zqxfg[QR] = zqxfg[QR] + zmelt;
          sa_sr = sa_sr + zmelt;
        }
      }
    }

    // 4.4b freezing of rain (:1864-1908)
    if (CLOUDSC_RUN(AB_MELT) && zqx[QR] > zepsec) {
      if (cold && cs.t_prev > c.rtt) {
        const real tot = fmax(zqx[QS] + zqx[QR], zepsec);
        cs.rainfrac = cl_div_p<real>(c, zqx[QR], tot);
      }
      if (ztp1 < c.rtt) {
        real zfrzmax;
        if (cs.rainfrac > R(0.8)) {
          const real zlambda = cl_pow<real>(c, cl_div_p<real>(c, c.rcl_fac1, (zrho * zqx[QR])), c.rcl_fac2);
          const real ztemp = c.rcl_fzrab * (ztp1 - c.rtt);
          const real zfrz = ((c.ptsphy * (cl_div_p<real>(c, c.rcl_const5r, zrho))) * (cl_exp<real>(c, ztemp) - R(1.0))) * cl_pow<real>(c, zlambda, c.rcl_const6r);
          zfrzmax = fmax(zfrz, R(0.0));
        } else {
          const real zcons1 = fabs(cl_div_known_p<real>(c, (c.ptsphy * (R(1.0) + R(0.5) * (c.rtt - ztp1))), c.rtaumel, c.rtaumel_rcp));
          zfrzmax = fmax(((c.rtt - ztp1) * zcons1) * c.zrldcp, R(0.0));
        }
        if (zfrzmax > zepsec) {
          const real zfrz = fmin(zqx[QR], zfrzmax); sa_sr = sa_sr - zfrz;
        }
      }
    }
    // 4.4c freezing of liquid (:1913-1928)
    {
      const real zfrzmax = fmax((c.rthomo - ztp1) * c.zrldcp, R(0.0));
      if (CLOUDSC_RUN(AB_MELT) && zfrzmax > zepsec && zqxfg[QL] > zepsec) {
        const real zfrz = fmin(zqxfg[QL], zfrzmax);
        sa_li = sa_li + zfrz;
      }
    }

    CLOUDSC_MID_HOOK(5);
    // 4.5 evaporation of rain, Abel and Boutle (:1982-2040).  The humidity
    // threshold zzrh0, zqsliq and zqe are pure functions of values fixed by now
    // (cs.zcovpmax is not changed by either evaporation): they are evaluated
    // inside the precipitation tests that guard their only uses, so a wave
    // without rain or snow skips their divisions.  Same operations, same bits.
    auto zzrh0_of = [&]() {
      return fmin(fmax(c.rprecrhmax + cl_div_p<real>(c, ((R(1.0) - c.rprecrhmax) * cs.zcovpmax), r_1mza), c.rprecrhmax), R(1.0));
    };
    if (CLOUDSC_RUN(AB_EVAP) && zcovpclr > zepsec && zqxfg[QR] > zepsec) {
      const real zfoeeliqt = fmin(cl_div_p<real>(c, (c.r2es * e_liq), r_pap), R(0.5));
      const real zqsliq = cl_div_p<real>(c, zfoeeliqt, (R(1.0) - c.retv * zfoeeliqt));
      const real zzrh = fmin(R(0.8), zzrh0_of());
      const real zqe = fmax(R(0.0), fmin(zqx[QV], zqsliq));
      if (zqe < zzrh * zqsliq) {
        const real zpreclr = cl_div_p<real>(c, zqxfg[QR], cs.zcovptot);
        const real zfallcorr = cl_pow<real>(c, cl_div_p<real>(c, c.rdensref, zrho), R(0.4));
        const real zesatliq = c.rv_rd * (c.r2es * e_liq);
        const real zlambda = cl_pow<real>(c, cl_div_p<real>(c, c.rcl_fac1, (zrho * zpreclr)), c.rcl_fac2);
        const real zevap_denom = c.rcl_cdenom1 * zesatliq - c.rcl_cdenom2 * ztp1 * zesatliq + (c.rcl_cdenom3 * cl_pow<real>(c, ztp1, R(3.0))) * pap_k;
        const real zcorr2 = cl_div_p<real>(c, (cl_pow<real>(c, cl_div_lit_p<real>(c, ztp1, R(273.0)), R(1.5)) * R(393.0)), (ztp1 + R(120.0)));
        const real zsubsat = fmax(zzrh * zqsliq - zqe, R(0.0));
        const real zbeta = ((((cl_div_p<real>(c, R(0.5), zqsliq)) * (ztp1 * ztp1)) * zesatliq) * c.rcl_const1r) * (cl_div_p<real>(c, zcorr2, zevap_denom)) *
                           (cl_div_p<real>(c, R(0.78), cl_pow<real>(c, zlambda, c.rcl_const4r)) + cl_div_p<real>(c, (c.rcl_const2r * cl_sqrt_p<real>(c, zrho * zfallcorr)), (cl_sqrt_p<real>(c, zcorr2) * cl_pow<real>(c, zlambda, c.rcl_const3r))));
        const real zdenom = R(1.0) + zbeta * c.ptsphy;
        const real zdpevap = cl_div_p<real>(c, (((zcovpclr * zbeta) * c.ptsphy) * zsubsat), zdenom);
        const real zevap = fmin(zdpevap, zqxfg[QR]);
        sa_rv = sa_rv + zevap;
        cs.zcovptot = fmax(c.rcovpmin, cs.zcovptot - fmax(R(0.0), cl_div_p<real>(c, ((cs.zcovptot - za) * zevap), zqxfg[QR])));
        zqxfg[QR] = zqxfg[QR] - zevap;
      }
    }
    // 4.5 evaporation of snow, Sundqvist (:2048-2087)
#if CLOUDSC_PHYSICS_SPP
    const real spp_rg_rpecons = spp.rg_rpecons(c);
    if (CLOUDSC_RUN(AB_EVAP) && zcovpclr > zepsec && zqxfg[QS] > zepsec) {
      const real zzrh = zzrh0_of();
#else
    if (CLOUDSC_RUN(AB_EVAP) && zcovpclr > zepsec && zqxfg[QS] > zepsec) {
      const real zzrh = zzrh0_of();
#endif
      real zqe = cl_div_p<real>(c, (zqx[QV] - za * zqsice), r_1mza);
      zqe = fmax(R(0.0), fmin(zqe, zqsice));
      if (zqe < zzrh * zqsice) {
        const real x = cs.zcovptot * zdtgdp;
        const real zpreclr = cl_div_p<real>(c, (zqxfg[QS] * zcovpclr), copysign(fmax(fabs(x), zepsilon), x));
        const real zbeta1 = cl_div_p<real>(c, ((cl_div_known_p<real>(c, cl_sqrt_p<real>(c, cl_div_p<real>(c, pap_k, cc.paph_sfc)), c.rvrfactor, c.rvrfactor_rcp)) * zpreclr), fmax(zcovpclr, zepsec));
#if CLOUDSC_PHYSICS_SPP
        const real zbeta = spp_rg_rpecons * cl_pow<real>(c, zbeta1, R(0.5777));
#else
        const real zbeta = c.rg_rpecons * cl_pow<real>(c, zbeta1, R(0.5777));
#endif
        const real zdenom = R(1.0) + (zbeta * c.ptsphy) * zcorqsice;
        const real zdpr = ((cl_div_p<real>(c, ((zcovpclr * zbeta) * (zqsice - zqe)), zdenom)) * zdp) * c.zrg_r;
        const real zdpevap = zdpr * zdtgdp;
        const real zevap = fmin(zdpevap, zqxfg[QS]);
        sa_sv = sa_sv + zevap;
        cs.zcovptot = fmax(c.rcovpmin, cs.zcovptot - fmax(R(0.0), cl_div_p<real>(c, ((cs.zcovptot - za) * zevap), zqxfg[QS])));
        zqxfg[QS] = zqxfg[QS] - zevap;
      }
    }
    // evaporate small precipitation amounts (:2144-2158)
    if (zqxfg[QR] < c.rlmin) { sa_rv = sa_rv + zqxfg[QR]; }
    if (zqxfg[QS] < c.rlmin) { sa_sv = sa_sv + zqxfg[QS]; }

    // 5.1 cloud cover (:2168-2180)
    real zanew = cl_div_p<real>(c, (za + zsolac), (R(1.0) + zsolab));
    zanew = fmin(zanew, R(1.0));
    if (zanew < c.ramin) zanew = R(0.0);
    const real zda = zanew - zaorig;
    cs.zanewm1 = zanew;
    // the hook: the k-caching kernel issues the next level's first-consumed
    // loads here (PF 3), after the physics' peak of live temporaries
    CLOUDSC_MID_HOOK(0);

    // 5.2 truncate explicit sinks, species in order (:2233-2286).
    // Column m of zsolqa (zsolqa[n][m], n=0..4) in C indexing; for each m the
    // sum runs n = ql, qi, qr, qs, qv and every negative entry scales
    // zsolqa[n][m] and its transpose zsolqa[m][n] (the diagonal twice).
    // The structurally-zero entries are kept as literal zeros so the
    // summation order (and hence rounding) matches the dense reference.
    // Where the sinks do not exceed what is there, max(-psum, zmm) is zmm and
    // the reference's ratio zmm/zmm is exactly 1 (zmm >= zepsec, finite): its
    // scaling multiplies by 1 and changes no bit, so the division and the
    // scaling run only where they can change something (a wave skips them
    // when none of its columns needs them).
    {
      real z = R(0.0), psum, zrat;
      // m = ql: zsolqa[n][ql] = {ll, il, rl, sl, vl}
      psum = R(0.0) + sa_ll; psum = psum + (-sa_li); psum = psum + (-sa_lr); psum = psum + (-sa_ls); psum = psum + (-sa_lv);
      {
        const real zmm = fmax(zqx[QL], zepsec), den = fmax(R(0.0) - psum, zmm);
        if (CLOUDSC_RUN(AB_TRUNC) && (den != zmm || zmm == (real)__builtin_inf())) {   // else zrat = 1: identity
          zrat = cl_div_p<real>(c, zmm, den);
          if (sa_ll < R(0.0)) { sa_ll = sa_ll * zrat; sa_ll = sa_ll * zrat; }
          if (-sa_li < R(0.0)) sa_li = sa_li * zrat;
          if (-sa_lr < R(0.0)) sa_lr = sa_lr * zrat;
          if (-sa_ls < R(0.0)) sa_ls = sa_ls * zrat;
          if (-sa_lv < R(0.0)) sa_lv = sa_lv * zrat;
        }
      }
      // m = qi: {li, ii, ri, si(0), vi}
      psum = R(0.0) + sa_li; psum = psum + sa_ii; psum = psum + (-sa_ir); psum = psum + z; psum = psum + (-sa_iv);
      {
        const real zmm = fmax(zqx[QI], zepsec), den = fmax(R(0.0) - psum, zmm);
        if (CLOUDSC_RUN(AB_TRUNC) && (den != zmm || zmm == (real)__builtin_inf())) {   // else zrat = 1: identity
          zrat = cl_div_p<real>(c, zmm, den);
          if (sa_li < R(0.0)) sa_li = sa_li * zrat;
          if (sa_ii < R(0.0)) { sa_ii = sa_ii * zrat; sa_ii = sa_ii * zrat; }
          if (-sa_ir < R(0.0)) sa_ir = sa_ir * zrat;
          if (-sa_iv < R(0.0)) sa_iv = sa_iv * zrat;
        }
      }
      // m = qr: {lr, ir, rr, sr, vr}
      psum = R(0.0) + sa_lr; psum = psum + sa_ir; psum = psum + sa_rr; psum = psum + sa_sr; psum = psum + (-sa_rv);
      {
        const real zmm = fmax(zqx[QR], zepsec), den = fmax(R(0.0) - psum, zmm);
        if (CLOUDSC_RUN(AB_TRUNC) && (den != zmm || zmm == (real)__builtin_inf())) {   // else zrat = 1: identity
          zrat = cl_div_p<real>(c, zmm, den);
          if (sa_lr < R(0.0)) sa_lr = sa_lr * zrat;
          if (sa_ir < R(0.0)) sa_ir = sa_ir * zrat;
          if (sa_rr < R(0.0)) { sa_rr = sa_rr * zrat; sa_rr = sa_rr * zrat; }
          if (sa_sr < R(0.0)) sa_sr = sa_sr * zrat;
          if (-sa_rv < R(0.0)) sa_rv = sa_rv * zrat;
        }
      }
      // m = qs: {ls, is(0), rs, ss, vs}
      psum = R(0.0) + sa_ls; psum = psum + z; psum = psum + (-sa_sr); psum = psum + sa_ss; psum = psum + (-sa_sv);
      {
        const real zmm = fmax(zqx[QS], zepsec), den = fmax(R(0.0) - psum, zmm);
        if (CLOUDSC_RUN(AB_TRUNC) && (den != zmm || zmm == (real)__builtin_inf())) {   // else zrat = 1: identity
          zrat = cl_div_p<real>(c, zmm, den);
          if (sa_ls < R(0.0)) sa_ls = sa_ls * zrat;
          if (-sa_sr < R(0.0)) sa_sr = sa_sr * zrat;
          if (sa_ss < R(0.0)) { sa_ss = sa_ss * zrat; sa_ss = sa_ss * zrat; }
          if (-sa_sv < R(0.0)) sa_sv = sa_sv * zrat;
        }
      }
      // m = qv: {lv, iv, rv, sv, vv(0)}
      psum = R(0.0) + sa_lv; psum = psum + sa_iv; psum = psum + sa_rv; psum = psum + sa_sv; psum = psum + z;
      {
        const real zmm = fmax(zqx[QV], zepsec), den = fmax(R(0.0) - psum, zmm);
        if (CLOUDSC_RUN(AB_TRUNC) && (den != zmm || zmm == (real)__builtin_inf())) {   // else zrat = 1: identity
          zrat = cl_div_p<real>(c, zmm, den);
          if (sa_lv < R(0.0)) sa_lv = sa_lv * zrat;
          if (sa_iv < R(0.0)) sa_iv = sa_iv * zrat;
          if (sa_rv < R(0.0)) sa_rv = sa_rv * zrat;
          if (sa_sv < R(0.0)) sa_sv = sa_sv * zrat;
        }
      }
    }

    // 5.2.2 implicit solver (:2294-2397).  With the zsolqb sparsity above,
    //   zqlhs = I + diag(fallsink) + diag(row sums of zsolqb) - offdiag(zsolqb)
    // has off-diagonal entries only at [ql][qs] and [qi][qs] (C indexing), so
    // the unpivoted LU leaves every multiplier but those two at (signed) zero
    // and the forward/back substitutions reduce to the terms below.  The
    // skipped updates are x - (+/-0)*y == x exactly, so the results are
    // bit-identical to the dense elimination for finite data.
    {
      // RHS: zqxn[m] = zqx[m] + sum_n zsolqa[n][m], n ascending from 0.0
      real ex;
      ex = R(0.0) + sa_ll; ex = ex + (-sa_li); ex = ex + (-sa_lr); ex = ex + (-sa_ls); ex = ex + (-sa_lv);
      real qn_l = zqx[QL] + ex;
      ex = R(0.0) + sa_li; ex = ex + sa_ii; ex = ex + (-sa_ir); ex = ex + R(0.0); ex = ex + (-sa_iv);
      real qn_i = zqx[QI] + ex;
      ex = R(0.0) + sa_lr; ex = ex + sa_ir; ex = ex + sa_rr; ex = ex + sa_sr; ex = ex + (-sa_rv);
      real qn_r = zqx[QR] + ex;
      ex = R(0.0) + sa_ls; ex = ex + R(0.0); ex = ex + (-sa_sr); ex = ex + sa_ss; ex = ex + (-sa_sv);
      real qn_s = zqx[QS] + ex;
      ex = R(0.0) + sa_lv; ex = ex + sa_iv; ex = ex + sa_rv; ex = ex + sa_sv; ex = ex + R(0.0);
      real qn_v = zqx[QV] + ex;
      // LHS diagonal: 1 + fallsink + sum_o zsolqb[m][o] (o ascending)
      real d_l = R(1.0) + R(0.0);
      d_l = d_l + sb_ll; d_l = d_l + R(0.0); d_l = d_l + R(0.0); d_l = d_l + sb_ls; d_l = d_l + R(0.0);
      real d_i = R(1.0) + fsink_i;
      d_i = d_i + R(0.0); d_i = d_i + sb_ii; d_i = d_i + R(0.0); d_i = d_i + sb_is; d_i = d_i + R(0.0);
      const real d_r = R(1.0) + fsink_r;   // + five zeros
      const real d_s = R(1.0) + fsink_s;
      // off-diagonals zqlhs[ql][qs] = -sb_ls, zqlhs[qi][qs] = -sb_is; LU scales row-wise by
      // the pivot of the eliminating column: zqlhs[n][m] /= zqlhs[n][n] for m > n.
      const Recip<real> r_dl = cl_recip_p<real>(c, d_l), r_di = cl_recip_p<real>(c, d_i);
      const real u_ls = cl_div_p<real>(c, (-sb_ls), r_dl);    // zqlhs[ql][qs] after jn = ql
      const real u_is = cl_div_p<real>(c, (-sb_is), r_di);    // zqlhs[qi][qs] after jn = qi
      // forward substitution (step 1): zqxn[qs] -= zqlhs[ql][qs]*zqxn[ql] + zqlhs[qi][qs]*zqxn[qi]
      qn_s = qn_s - u_ls * qn_l;
      qn_s = qn_s - u_is * qn_i;
      // back substitution (step 2): vapour and the diagonal solves
      // qn_v = qn_v / zqlhs[qv][qv] with a pivot of exactly 1: x / 1 == x in IEEE arithmetic
      // (signed zeros and NaN included), so the division is dropped
      if (CLOUDSC_RUN(AB_SOLVE)) {
        qn_s = cl_div_p<real>(c, qn_s, d_s);
        qn_r = cl_div_p<real>(c, qn_r, d_r);
        qn_i = cl_div_p<real>(c, qn_i, r_di);
        qn_l = cl_div_p<real>(c, qn_l, r_dl);
      }
      // no small values (:2402-2412)
      if (qn_l < zepsec) { qn_v = qn_v + qn_l; qn_l = R(0.0); }
      if (qn_i < zepsec) { qn_v = qn_v + qn_i; qn_i = R(0.0); }
      if (qn_r < zepsec) { qn_v = qn_v + qn_r; qn_r = R(0.0); }
      if (qn_s < zepsec) { qn_v = qn_v + qn_s; qn_s = R(0.0); }
      zqxn[QL] = qn_l; zqxn[QI] = qn_i; zqxn[QR] = qn_r; zqxn[QS] = qn_s;
      cs.qxnm1_l = qn_l; cs.qxnm1_i = qn_i;

      // 5.3 precipitation fluxes to the next level (:2430-2448)
      cs.pfx_i = (fsink_i * qn_i) * zrdtgdp;
      cs.pfx_r = (fsink_r * qn_r) * zrdtgdp;
      cs.pfx_s = (fsink_s * qn_s) * zrdtgdp;
      if (cs.pfx_s + cs.pfx_r < zepsec) cs.zcovptot = R(0.0);

      // 6. tendencies (:2456-2506)
      {
        const real fq_l = psup_l + conv_src_l + R(0.0) - (R(0.0) + conv_sink) * qn_l;
        ttend = ttend + (c.ralvdcp * (qn_l - zqx[QL] - fq_l)) * c.zqtmst;
        const real fq_i = psup_i + conv_src_i + fsrc_i - (fsink_i + conv_sink) * qn_i;
        ttend = ttend + (c.ralsdcp * (qn_i - zqx[QI] - fq_i)) * c.zqtmst;
        const real fq_r = R(0.0) + R(0.0) + fsrc_r - (fsink_r + R(0.0)) * qn_r;
        ttend = ttend + (c.ralvdcp * (qn_r - zqx[QR] - fq_r)) * c.zqtmst;
        const real fq_s = R(0.0) + R(0.0) + fsrc_s - (fsink_s + R(0.0)) * qn_s;
        ttend = ttend + (c.ralsdcp * (qn_s - zqx[QS] - fq_s)) * c.zqtmst;
      }
  #pragma unroll
      for (int m = 0; m < 4; m++) ctend[m] = R(0.0) + (zqxn[m] - zqx0[m]) * c.zqtmst;
      qtend = qtend + (qn_v - zqx[QV]) * c.zqtmst;
      atend = R(0.0) + zda * c.zqtmst;
      po.zcovptot_out = cs.zcovptot;
    }
}
