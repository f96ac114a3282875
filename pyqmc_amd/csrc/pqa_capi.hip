// pyqmc_amd C ABI implementation (host side): parameters, the walker state and the protocol entry points.  See
// include/pyqmc_amd.h for the contract; pqa_create.hip builds and destroys the handle.
#include "pqa_internal.hpp"
#include "pqa_stage.hpp"

// ---------------------------------------------------------------- parameters
extern "C" int pqa_set_param(pqa_handle_t* h, const char* name, const double* data, int64_t n) {
  h->dmc.old_valid = false;  // (the state pqa_dmc_continue refers to is gone)
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const std::string k(name);
  auto expect = [&](int64_t want) { return n == want; };
  if (k == "acoeff") {
    if (!expect((int64_t)h->natom * h->na * 2)) FAIL("acoeff size mismatch");
    HIPCHK(hipMemcpy(h->d_acoeff, data, n * sizeof(double), hipMemcpyDefault));
    TRY(jas_merge_tables(h));
  } else if (k == "bcoeff") {
    if (!expect((int64_t)h->nb * 3)) FAIL("bcoeff size mismatch");
    HIPCHK(hipMemcpy(h->d_bcoeff, data, n * sizeof(double), hipMemcpyDefault));
    TRY(jas_merge_tables(h));
  } else if (k == "ccoeff") {
    if (!h->has_j3 || !expect((int64_t)h->natom * h->na3 * h->na3 * h->nb3 * 3)) FAIL("ccoeff size mismatch");
    std::vector<double> host((size_t)n);
    HIPCHK(hipMemcpy(host.data(), data, n * sizeof(double), hipMemcpyDefault));
    TRY(set_c3(h, host.data()));
  } else if (k == "det_coeff") {
    if (!h->has_slater || !expect(h->ndet)) FAIL("det_coeff size mismatch");
    HIPCHK(hipMemcpy(h->d_detcoeff, data, n * sizeof(double), hipMemcpyDefault));
  } else if (k == "mo_coeff_alpha" || k == "mo_coeff_beta") {
    const int s = k == "mo_coeff_beta";
    if (!h->has_slater || !expect((int64_t)h->nao * h->nmo[s])) FAIL("mo_coeff size mismatch");
    std::vector<double> host((size_t)n);
    HIPCHK(hipMemcpy(host.data(), data, n * sizeof(double), hipMemcpyDefault));
    TRY(set_mo(h, s, host.data()));
  } else
    FAIL("unknown parameter name");
  h->saved_valid = false;
  return 0;
}

extern "C" int pqa_get_param(pqa_handle_t* h, const char* name, double* out, int64_t n) {
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const std::string k(name);
  const double* src = nullptr;
  int64_t want = 0;
  if (k == "acoeff") { src = h->d_acoeff; want = (int64_t)h->natom * h->na * 2; }
  else if (k == "bcoeff") { src = h->d_bcoeff; want = (int64_t)h->nb * 3; }
  else if (k == "det_coeff") { src = h->d_detcoeff; want = h->ndet; }
  else if (k == "mo_coeff_alpha") { src = h->d_mo[0]; want = (int64_t)h->nao * h->nmo[0]; }
  else if (k == "mo_coeff_beta") { src = h->d_mo[1]; want = (int64_t)h->nao * h->nmo[1]; }
  else if (k == "radial_table_info") {  // [number of table doubles, largest fit error relative to sum |c|] (build_radial_tables)
    if (n != 2) FAIL("parameter size mismatch");
    long used = 0;
    for (size_t q = 0; q + 1 < h->rt_shells.size(); q += 2)
      if (h->rt_shells[q] >= 0) used = std::max(used, (long)h->rt_shells[q] + (long)h->rt_shells[q + 1] * PQA_RT_REC);
    out[0] = (double)used; out[1] = h->rt_err;
    return 0;
  }
  else FAIL("unknown parameter name");
  if (n != want) FAIL("parameter size mismatch");
  HIPCHK(hipMemcpy(out, src, n * sizeof(double), hipMemcpyDefault));
  return 0;
}

extern "C" int pqa_eval_ao(pqa_handle_t* h, const double* pts, int64_t npts, int ncomp, double* out) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater) FAIL("handle has no orbital tables");
  if (ncomp != 1 && ncomp != 4 && ncomp != 5) FAIL("ncomp must be 1, 4 or 5");
  if (h->twist) FAIL("AO-only evaluation is not available for twisted cells (complex AOs); use pqa_eval_mo");
  if (npts <= 0) return 0;
  const size_t nout = (size_t)ncomp * npts * h->nao;
  TRY(ensure(h, h->b_pts, (size_t)npts * 3 * sizeof(double)));
  TRY(ensure(h, h->b_ao, nout * sizeof(double)));
  TRY(copy_in(h, h->b_pts.p, pts, (size_t)npts * 3 * sizeof(double)));
  const dim3 grid((unsigned)((npts + 63) / 64)), block(64);
  TRY(launch_ao(h, plain_points((const double*)h->b_pts.p, npts), npts, ncomp, (double*)h->b_ao.p));
  TRY(check_launch(h, "k_ao"));
  return copy_out(h, out, h->b_ao.p, nout * sizeof(double));
}

extern "C" int pqa_eval_mo(pqa_handle_t* h, int spin, const double* pts, int64_t npts, int ncomp, int use_mfma, double* out) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater) FAIL("handle has no orbital tables");
  if (ncomp != 1 && ncomp != 5) FAIL("ncomp must be 1 or 5");
  if (spin < 0 || spin > 1) FAIL("spin must be 0 or 1");
  if (npts <= 0 || h->nmo[spin] == 0) return 0;
  const int nmo = h->nmo[spin];
  const size_t nout = (size_t)ncomp * npts * nmo;
  h->saved_valid = false;
  TRY(ensure(h, h->b_pts, (size_t)npts * 3 * sizeof(double)));
  TRY(ensure(h, h->b_out, nout * sizeof(double)));
  TRY(copy_in(h, h->b_pts.p, pts, (size_t)npts * 3 * sizeof(double)));
  std::vector<double> host(nout);
  if (use_mfma) {
    TRY(ensure(h, h->b_motmp, nout * sizeof(double)));
    TRY(launch_orb(h, spin, plain_points((const double*)h->b_pts.p, npts), npts, ncomp, (double*)h->b_motmp.p));
    TRY(copy_out(h, host.data(), h->b_motmp.p, nout * sizeof(double)));
    std::vector<double> tr(nout);  // [p][c][j] -> [c][p][j]
    for (int64_t p = 0; p < npts; ++p)
      for (int c = 0; c < ncomp; ++c)
        memcpy(&tr[((size_t)c * npts + p) * nmo], &host[((size_t)p * ncomp + c) * nmo], nmo * sizeof(double));
    HIPCHK(hipMemcpy(out, tr.data(), nout * sizeof(double), hipMemcpyDefault));
    return 0;
  }
  const size_t nao_out = (size_t)ncomp * npts * h->nao;
  TRY(ensure(h, h->b_ao, nao_out * sizeof(double)));
  const dim3 grid((unsigned)((npts + 63) / 64)), block(64);
  TRY(launch_ao(h, plain_points((const double*)h->b_pts.p, npts), npts, ncomp, (double*)h->b_ao.p));
  const long rows = (long)ncomp * npts;
  hipLaunchKernelGGL((k_mo_valu<>), dim3((unsigned)((rows * nmo + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->b_ao.p,
                     (const double*)h->d_mo[spin], rows, h->nao, nmo, (double*)h->b_out.p);
  TRY(check_launch(h, "k_mo_valu"));
  return copy_out(h, out, h->b_out.p, nout * sizeof(double));
}

// ---------------------------------------------------------------- walker state
// The resident per-walker arrays, in the order pqa_resample gathers them: coordinates, per spin the inverses, determinant
// phases / logs and orbital cache, the two-body Jastrow sums, the three-body value.  ensure_walkers sizes them, pqa_resample
// gathers them into their alternate twins, recompute_range offsets the state pointers into them.
struct WalkerRow {
  DevBuf *cur, *alt;  // the array and its twin (pqa_resample's other half)
  size_t row;         // doubles per walker
  double** ptr;       // the SlaterState / JastrowState pointer the array backs (nullptr: none)
  bool has;           // the handle keeps this array
  bool jas_sum;       // a Jastrow sum: not gathered while jas_stale (recomputed before its next use)
};
static std::array<WalkerRow, 12> walker_rows(pqa_handle* h) {
  const size_t cf = h->cplx ? 2 : 1;
  const int nel[2] = {h->nup, h->ndn};
  std::array<WalkerRow, 12> r;
  int k = 0;
  r[k++] = {&h->b_x, &h->b_alt_x, (size_t)h->N * 3, &h->js.x, true, false};
  for (int s = 0; s < 2; ++s) {
    const size_t D = h->ndet_s[s], n = nel[s];
    r[k++] = {&h->b_T[s], &h->b_alt_T[s], cf * D * n * n, &h->st.T[s], h->has_slater, false};
    r[k++] = {&h->b_dsign[s], &h->b_alt_dsign[s], cf * D, &h->st.dsign[s], h->has_slater, false};
    r[k++] = {&h->b_dlog[s], &h->b_alt_dlog[s], D, &h->st.dlog[s], h->has_slater, false};
    r[k++] = {&h->b_cache[s], &h->b_alt_cache[s], n * 5 * h->nmo[s], &h->st.cache[s], h->has_slater, false};
  }
  r[k++] = {&h->b_aval, &h->b_alt_aval, (size_t)h->natom * h->na * 2, &h->js.avalues, h->has_j2, true};
  r[k++] = {&h->b_bval, &h->b_alt_bval, (size_t)h->nb * 3, &h->js.bvalues, h->has_j2, true};
  r[k++] = {&h->b_j3u, &h->b_alt_j3u, 1, nullptr, true, false};  // (always sized: pqa_j3_value's output)
  return r;
}

static int ensure_walkers(pqa_handle* h, long W) {
  if (W <= 0) FAIL("number of walkers must be positive");
  if (W != h->W) {  // (the deferred ECP point totals and the kernel-choice hints describe the shard they were measured on: ADVICE r5)
    h->en.hint_valid = false; h->en.last_dev[0] = h->en.last_dev[1] = nullptr;
    if (h->en.last_points < 0) h->en.last_points = 0;
  }
  h->W = W;
  h->saved_valid = false;
  for (const WalkerRow& r : walker_rows(h)) {
    if (!r.has) continue;
    TRY(ensure(h, *r.cur, (size_t)W * r.row * sizeof(double)));
    if (r.ptr) *r.ptr = (double*)r.cur->p;
  }
  // scratch, not state
  TRY(ensure(h, h->b_sign, (h->cplx ? 2 : 1) * W * sizeof(double)));
  TRY(ensure(h, h->b_log, W * sizeof(double)));
  TRY(ensure(h, h->b_ju, W * sizeof(double)));
  TRY(ensure(h, h->b_mask, W));
  return 0;
}

int jas_refresh(pqa_handle* h) {
  if (h->has_j2 && h->jas_stale && h->W > 0) {
    hipLaunchKernelGGL((k_jastrow_recompute<>), dim3((unsigned)h->W), dim3(64), 0, h->stream, h->S, h->js);
    TRY(check_launch(h, "k_jastrow_recompute"));
  }
  h->jas_stale = false;
  return 0;
}

int slater_rebuild(pqa_handle* h) {  // cache + inverse + determinants from js.x
  const int nel[2] = {h->nup, h->ndn};
  for (int s = 0; s < 2; ++s) {
    if (nel[s] == 0) {  // an empty spin channel (fully polarised system): the determinant of the 0 x 0 matrix is 1
      const size_t nd = (size_t)h->W * std::max(h->ndet_s[s], 1);
      std::vector<double> one((h->cplx ? 2 : 1) * nd, 0.0);
      for (size_t k = 0; k < nd; ++k) one[(h->cplx ? 2 : 1) * k] = 1.0;
      HIPCHK(hipStreamSynchronize(h->stream));
      HIPCHK(hipMemcpy(h->st.dsign[s], one.data(), one.size() * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipMemset(h->st.dlog[s], 0, nd * sizeof(double)));
      continue;
    }
    PointAddr pa;
    pa.base = h->js.x + (size_t)(s ? h->nup : 0) * 3;
    pa.group = nel[s];
    pa.group_stride = (long)h->N * 3;
    TRY(launch_orb(h, s, pa, h->W * nel[s], 5, h->st.cache[s]));
    const size_t lds = (h->cplx ? 2 : 1) * ((size_t)nel[s] * (nel[s] + 1)) * sizeof(double) + (size_t)nel[s] * sizeof(int) + 16;
    if (!h->cplx && lds > 64 * 1024 && !h->invert_attr) {  // (91 electrons of a spin and more: past the default dynamic-LDS limit)
      HIPCHK(hipFuncSetAttribute((const void*)k_build_invert<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      h->invert_attr = true;
    }
    if (h->cplx && nel[s] > PQA_MAXN_FAST) {  // the complex tile does not fit LDS: scratch matrices in global memory, <= 512 MB per pass
      const size_t per = (size_t)2 * nel[s] * (nel[s] + 1) * sizeof(double) * h->ndet_s[s];
      const long wchunk = std::max<long>(1, std::min<long>(h->W, (long)(((size_t)512 << 20) / per)));
      TRY(ensure(h, h->b_ao, (size_t)wchunk * per));
      for (long w0 = 0; w0 < h->W; w0 += wchunk) {
        const long nw = std::min(wchunk, h->W - w0);
        hipLaunchKernelGGL((k_build_invert_cg<>), dim3((unsigned)(nw * h->ndet_s[s])), dim3(64), (size_t)nel[s] * sizeof(int) + 16, h->stream, h->S, h->st, s, w0,
                           (double*)h->b_ao.p);
      }
    } else
    if (h->cplx) hipLaunchKernelGGL((k_build_invert_c<>), dim3((unsigned)(h->W * h->ndet_s[s])), dim3(64), lds, h->stream, h->S, h->st, s, h->W);
    else hipLaunchKernelGGL((k_build_invert<>), dim3((unsigned)(h->W * h->ndet_s[s])), dim3(64), lds, h->stream, h->S, h->st, s, h->W);
    TRY(check_launch(h, "k_build_invert"));
  }
  return 0;
}

int slater_value_dev(pqa_handle* h) {
  if (h->cplx) hipLaunchKernelGGL((k_slater_value_c<>), dim3((unsigned)h->W), dim3(64), 0, h->stream, h->S, h->st, (double*)h->b_sign.p, (double*)h->b_log.p);
  else hipLaunchKernelGGL((k_slater_value<>), dim3((unsigned)h->W), dim3(64), 0, h->stream, h->S, h->st, (double*)h->b_sign.p, (double*)h->b_log.p);
  return check_launch(h, "k_slater_value");
}

extern "C" int pqa_slater_recompute(pqa_handle_t* h, const double* configs, int64_t W, double* sign, double* logabs) {
  h->dmc.old_valid = false;  // (the state pqa_dmc_continue refers to is gone)
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater) FAIL("handle has no Slater factor");
  if (!h->has_jastrow || h->W != W) {
    TRY(ensure_walkers(h, W));
    TRY(copy_in(h, h->js.x, configs, (size_t)W * h->N * 3 * sizeof(double)));
    TRY(slater_rebuild(h));
  } else {
    // the Jastrow factor owns the stored walker coordinates; evaluate from a scratch copy
    h->saved_valid = false;
    double* keep = h->js.x;
    TRY(ensure(h, h->b_pts, (size_t)W * h->N * 3 * sizeof(double)));
    TRY(copy_in(h, h->b_pts.p, configs, (size_t)W * h->N * 3 * sizeof(double)));
    h->js.x = (double*)h->b_pts.p;
    int rc = slater_rebuild(h);
    h->js.x = keep;
    if (rc) return rc;
  }
  return pqa_slater_value(h, sign, logabs);
}

extern "C" int pqa_slater_value(pqa_handle_t* h, double* sign, double* logabs) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater || h->W == 0) FAIL("Slater state not initialised (call recompute)");
  TRY(slater_value_dev(h));
  TRY(copy_in(h, sign, h->b_sign.p, (h->cplx ? 2 : 1) * h->W * sizeof(double)));
  return copy_out(h, logabs, h->b_log.p, h->W * sizeof(double));
}

extern "C" int pqa_slater_eval(pqa_handle_t* h, int e, const double* pts, int64_t nrow, int npt, const int32_t* widx,
                               int ncomp, int keep_saved, double* out) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater || h->W == 0) FAIL("Slater state not initialised (call recompute)");
  if (ncomp != 1 && ncomp != 5) FAIL("ncomp must be 1 or 5");
  StagedPoints in;
  TRY(stage_eval(h, "pqa_slater_eval", h->W, e, pts, nrow, npt, widx, 0, &in));
  if (!in.P) return 0;
  const int s = e >= h->nup, nmo = h->nmo[s];
  const long P = in.P;
  const int* dw = in.widx;
  h->saved_valid = false;
  TRY(ensure(h, h->b_motmp, (size_t)P * ncomp * nmo * sizeof(double)));
  const size_t cf = h->cplx ? 2 : 1;
  TRY(ensure(h, h->b_out, cf * (size_t)P * ncomp * sizeof(double)));
  TRY(launch_orb(h, s, plain_points(in.pts, P), P, ncomp, (double*)h->b_motmp.p));
  const dim3 grid((unsigned)nrow), block(64);
  if (h->cplx) {
    if (ncomp == 1)
      hipLaunchKernelGGL(k_slater_eval_c<1>, grid, block, 2 * lds_det(h, 1), h->stream, h->S, h->st, e, (const double*)h->b_motmp.p,
                         (long)nrow, npt, dw, (double*)h->b_out.p);
    else
      hipLaunchKernelGGL(k_slater_eval_c<5>, grid, block, 2 * lds_det(h, 5), h->stream, h->S, h->st, e, (const double*)h->b_motmp.p,
                         (long)nrow, npt, dw, (double*)h->b_out.p);
  } else
  if (ncomp == 1)
    hipLaunchKernelGGL(k_slater_eval<1>, grid, block, lds_det(h, 1), h->stream, h->S, h->st, e, (const double*)h->b_motmp.p,
                       (long)nrow, npt, dw, (double*)h->b_out.p);
  else
    hipLaunchKernelGGL(k_slater_eval<5>, grid, block, lds_det(h, 5), h->stream, h->S, h->st, e, (const double*)h->b_motmp.p,
                       (long)nrow, npt, dw, (double*)h->b_out.p);
  TRY(check_launch(h, "k_slater_eval"));
  TRY(copy_out(h, out, h->b_out.p, cf * (size_t)P * ncomp * sizeof(double)));
  if (keep_saved && npt == 1 && !widx && ncomp == 5) { h->saved_valid = true; h->saved_e = e; }
  return 0;
}

extern "C" int pqa_testvalue_many(pqa_handle_t* h, const int32_t* es, int ne, const double* pts, int64_t nrow, const int32_t* widx,
                                  int factors, double* out) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("state not initialised (call recompute)");
  if (nrow <= 0 || ne <= 0) return 0;
  if ((factors & 1) && !h->has_slater) FAIL("handle has no Slater factor");
  if ((factors & 2) && !h->has_j2) FAIL("handle has no two-body Jastrow factor");
  if ((factors & 4) && !h->has_j3) FAIL("handle has no three-body Jastrow factor");
  if (!(factors & 7)) FAIL("no factor selected");
  const int* des;
  StagedPoints in;
  TRY(stage_points(h, "pqa_testvalue_many", h->W, pts, nrow, 1, widx, &in));
  TRY(stage_electrons(h, "pqa_testvalue_many", es, ne, &des));
  const int* dw = in.widx;
  h->saved_valid = false;
  const size_t cf = h->cplx ? 2 : 1;  // complex handles return (re, im) pairs
  TRY(ensure(h, h->b_out, cf * nrow * ne * sizeof(double)));
  if (factors & 1)
    for (int s = 0; s < 2; ++s) {
      TRY(ensure(h, h->b_emo[s], (size_t)nrow * std::max(h->nmo[s], 1) * sizeof(double)));
      TRY(launch_orb(h, s, plain_points(in.pts, nrow), nrow, 1, (double*)h->b_emo[s].p));
    }
  if (h->cplx)
    hipLaunchKernelGGL(k_testvalue_many<true>, dim3((unsigned)nrow), dim3(64), 2 * lds_det(h, 1), h->stream, h->S, h->st, h->js,
                       des, ne, in.pts, (const double*)h->b_emo[0].p,
                       (const double*)h->b_emo[1].p, (long)nrow, dw, factors, (double*)h->b_out.p);
  else
    hipLaunchKernelGGL(k_testvalue_many<false>, dim3((unsigned)nrow), dim3(64), lds_det(h, 1), h->stream, h->S, h->st, h->js,
                       des, ne, in.pts, (const double*)h->b_emo[0].p,
                       (const double*)h->b_emo[1].p, (long)nrow, dw, factors, (double*)h->b_out.p);
  TRY(check_launch(h, "k_testvalue_many"));
  return copy_out(h, out, h->b_out.p, cf * nrow * ne * sizeof(double));
}

extern "C" int pqa_slater_pgradient(pqa_handle_t* h, double* d_det, double* d_mo_up, double* d_mo_dn) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater || h->W == 0) FAIL("Slater state not initialised (call recompute)");
  const long W = h->W;
  const size_t cf = h->cplx ? 2 : 1;  // complex handles: every output is complex, (re, im) interleaved; nmo below counts orbitals
  TRY(pgrad_det_dev(h));  // (with the sign / log of the determinant expansion -> b_sign, b_log, which k_pgrad_mo reads below)
  if (d_det) TRY(copy_out(h, d_det, h->b_pgdet.p, cf * W * h->ndet * sizeof(double)));
  double* outs[2] = {d_mo_up, d_mo_dn};
  if (!d_mo_up && !d_mo_dn) return 0;
  // AO values of every electron at its position: real, or for a twisted cell complex (two planes; the walkers of a twisted
  // handle are unfolded: k_ao_tw folds every point and gives it its wrap phase)
  const long ao_plane = W * h->N * (long)h->nao;
  const size_t nao_all = (size_t)ao_plane * (h->twist ? 2 : 1);
  if (nao_all * sizeof(double) > ((size_t)16 << 30)) FAIL("orbital-coefficient gradients need the AO values of all electrons: too many walkers for one call");
  TRY(ensure(h, h->b_ao, nao_all * sizeof(double)));
  const dim3 ga((unsigned)((W * h->N + 63) / 64));
  if (h->twist) hipLaunchKernelGGL((k_ao_tw<>), ga, dim3(64), 0, h->stream, h->S, (const double*)h->js.x, W * h->N, (double*)h->b_ao.p);
  else TRY(launch_ao(h, plain_points((const double*)h->js.x, W * h->N), W * h->N, 1, (double*)h->b_ao.p));
  TRY(check_launch(h, "k_ao"));
  for (int s = 0; s < 2; ++s) {
    const int n = s ? h->ndn : h->nup;
    if (!outs[s] || n == 0 || h->nmo[s] == 0) continue;
    const size_t nout = (size_t)W * h->nao * h->nmo[s];  // (complex: nmo[s] = 2 x orbitals, i.e. already the doubles of the complex result)
    TRY(ensure(h, h->b_out, nout * sizeof(double)));
    const size_t lds = cf * (size_t)h->ndet_s[s] * sizeof(double);
    if (!h->cplx) hipLaunchKernelGGL((k_pgrad_mo<>), dim3((unsigned)W), dim3(256), lds, h->stream, h->S, h->st, s,
                                     (const double*)h->b_ao.p, (const double*)h->b_pgdet.p, (const int*)h->d_colmap[s], (double*)h->b_out.p);
    else if (h->twist) hipLaunchKernelGGL(k_pgrad_mo_c<true>, dim3((unsigned)W), dim3(256), lds, h->stream, h->S, h->st, s, (const double*)h->b_ao.p, ao_plane,
                                          (const double*)h->b_pgdet.p, (const int*)h->d_colmap[s], (double*)h->b_out.p);
    else hipLaunchKernelGGL(k_pgrad_mo_c<false>, dim3((unsigned)W), dim3(256), lds, h->stream, h->S, h->st, s, (const double*)h->b_ao.p, ao_plane,
                            (const double*)h->b_pgdet.p, (const int*)h->d_colmap[s], (double*)h->b_out.p);
    TRY(check_launch(h, "k_pgrad_mo"));
    TRY(copy_out(h, outs[s], h->b_out.p, nout * sizeof(double)));
  }
  return 0;
}

extern "C" int pqa_slater_has_zero(pqa_handle_t* h, int spin, int* flag) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater || h->W == 0) FAIL("Slater state not initialised (call recompute)");
  TRY(ensure(h, h->b_flag, sizeof(int)));
  HIPCHK(hipMemsetAsync(h->b_flag.p, 0, sizeof(int), h->stream));
  const long count = h->W * h->ndet_s[spin];
  hipLaunchKernelGGL((k_has_zero<>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->st.dlog[spin], count, (int*)h->b_flag.p);
  TRY(check_launch(h, "k_has_zero"));
  return copy_out(h, flag, h->b_flag.p, sizeof(int));
}

extern "C" int pqa_slater_update(pqa_handle_t* h, int e, const double* epos, const uint8_t* mask, int use_saved) {
  h->dmc.old_valid = false;  // (the state pqa_dmc_continue refers to is gone)
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater || h->W == 0) FAIL("Slater state not initialised (call recompute)");
  const long W = h->W;
  const bool saved = use_saved && h->saved_valid && h->saved_e == e;  // the orbital rows are in b_motmp: the positions are not needed
  const double* dx = nullptr;
  const uint8_t* dm;
  TRY(stage_move(h, "pqa_slater_update", W, e, epos, mask, saved ? nullptr : &dx, &dm));
  const int s = e >= h->nup, nmo = h->nmo[s];
  if (!saved) {
    TRY(ensure(h, h->b_motmp, (size_t)W * 5 * nmo * sizeof(double)));
    TRY(launch_orb(h, s, plain_points(dx, W), W, 5, (double*)h->b_motmp.p));
  }
  h->saved_valid = false;
  if (h->cplx) hipLaunchKernelGGL((k_sm_update_c<>), dim3((unsigned)W), dim3(64), 2 * lds_sm(h), h->stream, h->S, h->st, e,
                                  (const double*)h->b_motmp.p, 5 * nmo, dm, 1);
  else hipLaunchKernelGGL((k_sm_update<>), dim3((unsigned)W), dim3(64), lds_sm(h), h->stream, h->S, h->st, e, (const double*)h->b_motmp.p,
                          5 * nmo, dm, 1);
  TRY(check_launch(h, "k_sm_update"));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int pqa_slater_get_state(pqa_handle_t* h, int spin, double* inverse, double* dets) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater || h->W == 0) FAIL("Slater state not initialised (call recompute)");
  const size_t W = h->W, D = h->ndet_s[spin], n = spin ? h->ndn : h->nup;
  HIPCHK(hipStreamSynchronize(h->stream));
  const size_t cf = h->cplx ? 2 : 1;  // complex: (re, im) interleaved in every output
  if (inverse) {
    std::vector<double> T(cf * W * D * n * n), inv(cf * W * D * n * n);
    HIPCHK(hipMemcpy(T.data(), h->st.T[spin], T.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t m = 0; m < W * D; ++m)
      for (size_t i = 0; i < n; ++i)
        for (size_t k = 0; k < n; ++k)
          for (size_t q = 0; q < cf; ++q) inv[((m * n + k) * n + i) * cf + q] = T[((m * n + i) * n + k) * cf + q];
    HIPCHK(hipMemcpy(inverse, inv.data(), inv.size() * sizeof(double), hipMemcpyDefault));
  }
  if (dets) {  // [phase (W,D) (complex: interleaved)] followed by [log (W,D)]
    std::vector<double> d((cf + 1) * W * D);
    HIPCHK(hipMemcpy(d.data(), h->st.dsign[spin], cf * W * D * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(d.data() + cf * W * D, h->st.dlog[spin], W * D * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dets, d.data(), d.size() * sizeof(double), hipMemcpyDefault));
  }
  return 0;
}

// ---------------------------------------------------------------- Jastrow
extern "C" int pqa_jastrow_recompute(pqa_handle_t* h, const double* configs, int64_t W, double* logval) {
  h->dmc.old_valid = false;  // (the state pqa_dmc_continue refers to is gone)
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_j2) FAIL("handle has no two-body Jastrow factor");
  if (h->W != W) TRY(ensure_walkers(h, W));
  h->jas_stale = false;
  TRY(copy_in(h, h->js.x, configs, (size_t)W * h->N * 3 * sizeof(double)));
  hipLaunchKernelGGL((k_jastrow_recompute<>), dim3((unsigned)W), dim3(64), 0, h->stream, h->S, h->js);
  TRY(check_launch(h, "k_jastrow_recompute"));
  return pqa_jastrow_value(h, logval);
}

extern "C" int pqa_jastrow_value(pqa_handle_t* h, double* logval) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_j2 || h->W == 0) FAIL("Jastrow state not initialised (call recompute)");
  TRY(jas_refresh(h));
  hipLaunchKernelGGL((k_jastrow_value<>), dim3((unsigned)h->W), dim3(64), 0, h->stream, h->S, h->js, (double*)h->b_ju.p);
  TRY(check_launch(h, "k_jastrow_value"));
  return copy_out(h, logval, h->b_ju.p, h->W * sizeof(double));
}

static int jastrow_eval_parts(pqa_handle_t* h, int parts, int e, const double* pts, int64_t nrow, int npt, const int32_t* widx,
                              int mode, double* out) {
  HIPCHK(hipSetDevice(h->device));
  if (!((parts & 1) ? h->has_j2 : h->has_j3) || h->W == 0) FAIL("Jastrow state not initialised (call recompute)");
  StagedPoints in;
  TRY(stage_eval(h, (parts & 1) ? "pqa_jastrow_eval" : "pqa_j3_eval", h->W, e, pts, nrow, npt, widx, mode, &in));
  if (!in.P) return 0;
  const size_t nout = mode == 0 ? (size_t)in.P : (size_t)4 * nrow;
  TRY(ensure(h, h->b_out, nout * sizeof(double)));
  hipLaunchKernelGGL((k_jastrow_eval<>), dim3((unsigned)nrow), dim3(64), lds_j3(h), h->stream, h->S, h->js, e, in.pts,
                     (long)nrow, npt, in.widx, mode, parts, (double*)h->b_out.p);
  TRY(check_launch(h, "k_jastrow_eval"));
  return copy_out(h, out, h->b_out.p, nout * sizeof(double));
}

extern "C" int pqa_jastrow_eval(pqa_handle_t* h, int e, const double* pts, int64_t nrow, int npt, const int32_t* widx,
                                int mode, double* out) {
  TRY(sync_aos(h));
  return jastrow_eval_parts(h, 1, e, pts, nrow, npt, widx, mode, out);
}

extern "C" int pqa_j3_eval(pqa_handle_t* h, int e, const double* pts, int64_t nrow, int npt, const int32_t* widx, int mode,
                           double* out) {
  TRY(sync_aos(h));
  return jastrow_eval_parts(h, 2, e, pts, nrow, npt, widx, mode, out);
}

static int j3_value_dev(pqa_handle* h) {
  hipLaunchKernelGGL((k_j3_value<>), dim3((unsigned)h->W), dim3(64), lds_j3(h), h->stream, h->S, h->js, (double*)h->b_j3u.p);
  return check_launch(h, "k_j3_value");
}

extern "C" int pqa_j3_value(pqa_handle_t* h, double* logval) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_j3 || h->W == 0) FAIL("three-body Jastrow state not initialised (call recompute)");
  TRY(j3_value_dev(h));
  return copy_out(h, logval, h->b_j3u.p, h->W * sizeof(double));
}

extern "C" int pqa_j3_pgradient(pqa_handle_t* h, double* d_ccoeff) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_j3 || h->W == 0) FAIL("three-body Jastrow state not initialised (call recompute)");
  TRY(j3_pgrad_dev(h));
  return copy_out(h, d_ccoeff, h->b_out.p, (size_t)h->W * h->natom * h->na3 * h->na3 * h->nb3 * 3 * sizeof(double));
}

extern "C" int pqa_j3_recompute(pqa_handle_t* h, const double* configs, int64_t W, double* logval) {
  h->dmc.old_valid = false;  // (the state pqa_dmc_continue refers to is gone)
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_j3) FAIL("handle has no three-body Jastrow factor");
  if (h->has_j2 && h->W == W) {  // the two-body factor owns the stored coordinates: evaluate from a scratch copy
    double* keep = h->js.x;
    TRY(ensure(h, h->b_pts, (size_t)W * h->N * 3 * sizeof(double)));
    TRY(copy_in(h, h->b_pts.p, configs, (size_t)W * h->N * 3 * sizeof(double)));
    h->js.x = (double*)h->b_pts.p;
    int rc = j3_value_dev(h);
    h->js.x = keep;
    if (rc) return rc;
    return copy_out(h, logval, h->b_j3u.p, W * sizeof(double));
  }
  if (h->W != W) TRY(ensure_walkers(h, W));
  TRY(copy_in(h, h->js.x, configs, (size_t)W * h->N * 3 * sizeof(double)));
  return pqa_j3_value(h, logval);
}

extern "C" int pqa_j3_update(pqa_handle_t* h, int e, const double* epos, const uint8_t* mask) {
  h->dmc.old_valid = false;  // (the state pqa_dmc_continue refers to is gone)
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_j3 || h->W == 0) FAIL("three-body Jastrow state not initialised (call recompute)");
  if (h->has_j2) {  // coordinates are moved by the two-body factor's update: nothing to stage, a bad index is an error all the same
    if (e < 0 || e >= h->N) FAIL("pqa_j3_update: electron index out of range");
    return 0;
  }
  const long W = h->W;
  const double* dx;
  const uint8_t* dm;
  TRY(stage_move(h, "pqa_j3_update", W, e, epos, mask, &dx, &dm));
  hipLaunchKernelGGL((k_move_x<>), dim3((unsigned)((W + 255) / 256)), dim3(256), 0, h->stream, h->js, h->N, e, dx, dm, W);
  TRY(check_launch(h, "k_move_x"));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int pqa_jastrow_update(pqa_handle_t* h, int e, const double* epos, const uint8_t* mask) {
  h->dmc.old_valid = false;  // (the state pqa_dmc_continue refers to is gone)
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_j2 || h->W == 0) FAIL("Jastrow state not initialised (call recompute)");
  const long W = h->W;
  const double* dx;
  const uint8_t* dm;
  TRY(stage_move(h, "pqa_jastrow_update", W, e, epos, mask, &dx, &dm));
  TRY(jas_refresh(h));
  hipLaunchKernelGGL((k_jastrow_update<>), dim3((unsigned)W), dim3(64), 0, h->stream, h->S, h->js, e, dx, dm);
  TRY(check_launch(h, "k_jastrow_update"));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---------------------------------------------------------------- product wave function: one call per protocol method
// MultiplyWF.gradient / gradient_value / gradient_laplacian and updateinternals (multiplywf.py:102-129) of a Slater x two-body-Jastrow
// product living on this handle.  The per-factor entries above cost a copy-in, a launch chain, a copy-out and a synchronisation EACH
// (tools/protocol_profile.py: ~60 us per call at 4096 walkers, seven calls per electron move of pyqmc.method.mc.vmc_worker); here
// the proposal goes in once and both factors' rows come back in one transfer.
extern "C" int pqa_wf_eval(pqa_handle_t* h, int e, const double* pts, int jmode, int keep_saved, double* out) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater || !h->has_j2 || h->has_j3 || h->cplx || h->W == 0) FAIL("pqa_wf_eval: a real Slater x two-body-Jastrow product with resident walkers");
  if (jmode != 1 && jmode != 2) FAIL("jmode: 1 (Jastrow gradient + value) or 2 (gradient + laplacian)");
  const long W = h->W;
  StagedPoints in;  // one point per resident walker
  TRY(stage_eval(h, "pqa_wf_eval", W, e, pts, W, 1, nullptr, jmode, &in));
  const int s = e >= h->nup, nmo = h->nmo[s];
  h->saved_valid = false;
  TRY(ensure(h, h->b_motmp, (size_t)W * 5 * nmo * sizeof(double)));
  TRY(ensure(h, h->b_out, (size_t)9 * W * sizeof(double)));
  TRY(launch_orb(h, s, plain_points(in.pts, W), W, 5, (double*)h->b_motmp.p));
  hipLaunchKernelGGL(k_slater_eval<5>, dim3((unsigned)W), dim3(64), lds_det(h, 5), h->stream, h->S, h->st, e, (const double*)h->b_motmp.p, W, 1,
                     (const int*)nullptr, (double*)h->b_out.p);
  hipLaunchKernelGGL((k_jastrow_eval<>), dim3((unsigned)W), dim3(64), lds_j3(h), h->stream, h->S, h->js, e, in.pts, W, 1,
                     (const int*)nullptr, jmode, 1, (double*)h->b_out.p + (size_t)5 * W);
  TRY(check_launch(h, "k_slater_eval / k_jastrow_eval"));
  TRY(copy_out(h, out, h->b_out.p, (size_t)9 * W * sizeof(double)));
  if (keep_saved) { h->saved_valid = true; h->saved_e = e; }
  return 0;
}

extern "C" int pqa_wf_update(pqa_handle_t* h, int e, const double* epos, const uint8_t* mask, int use_saved, int* has_zero) {
  h->dmc.old_valid = false;  // (the state pqa_dmc_continue refers to is gone)
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater || !h->has_j2 || h->has_j3 || h->cplx || h->W == 0) FAIL("pqa_wf_update: a real Slater x two-body-Jastrow product with resident walkers");
  const long W = h->W;
  const double* dx;
  const uint8_t* dm;
  TRY(stage_move(h, "pqa_wf_update", W, e, epos, mask, &dx, &dm));
  const int s = e >= h->nup, nmo = h->nmo[s];
  TRY(jas_refresh(h));
  if (!(use_saved && h->saved_valid && h->saved_e == e)) {
    TRY(ensure(h, h->b_motmp, (size_t)W * 5 * nmo * sizeof(double)));
    TRY(launch_orb(h, s, plain_points(dx, W), W, 5, (double*)h->b_motmp.p));
  }
  h->saved_valid = false;
  hipLaunchKernelGGL((k_sm_update<>), dim3((unsigned)W), dim3(64), lds_sm(h), h->stream, h->S, h->st, e, (const double*)h->b_motmp.p, 5 * nmo, dm, 1);
  hipLaunchKernelGGL((k_jastrow_update<>), dim3((unsigned)W), dim3(64), 0, h->stream, h->S, h->js, e, dx, dm);
  // slater.py:269-275 looks for a vanished determinant BEFORE an update; the flag of the state this call leaves is what the next
  // update of this spin needs (the caller keeps it), and it travels with the synchronisation the call ends with anyway
  TRY(ensure(h, h->b_flag, sizeof(int)));
  HIPCHK(hipMemsetAsync(h->b_flag.p, 0, sizeof(int), h->stream));
  const long count = W * h->ndet_s[s];
  hipLaunchKernelGGL((k_has_zero<>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->st.dlog[s], count, (int*)h->b_flag.p);
  TRY(check_launch(h, "k_sm_update / k_jastrow_update"));
  return copy_out(h, has_zero, h->b_flag.p, sizeof(int));
}

extern "C" int pqa_jastrow_get_state(pqa_handle_t* h, double* avalues, double* bvalues, double* configs) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("state not initialised (call recompute)");
  TRY(jas_refresh(h));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (avalues && h->has_j2) HIPCHK(hipMemcpy(avalues, h->js.avalues, (size_t)h->W * h->natom * h->na * 2 * sizeof(double), hipMemcpyDefault));
  if (bvalues && h->has_j2) HIPCHK(hipMemcpy(bvalues, h->js.bvalues, (size_t)h->W * h->nb * 3 * sizeof(double), hipMemcpyDefault));
  if (configs) HIPCHK(hipMemcpy(configs, h->js.x, (size_t)h->W * h->N * 3 * sizeof(double), hipMemcpyDefault));
  return 0;
}

// ---------------------------------------------------------------- fused path
static int wf_value_host(pqa_handle* h, double* sign, double* logabs) {
  const long W = h->W;
  const size_t cf = h->cplx ? 2 : 1;
  std::vector<double> sg(cf * W, 1.0), lg(W, 0.0), ju(W, 0.0);
  if (h->has_slater) {
    TRY(slater_value_dev(h));
    TRY(copy_in(h, sg.data(), h->b_sign.p, cf * W * sizeof(double)));
    TRY(copy_in(h, lg.data(), h->b_log.p, W * sizeof(double)));
  }
  std::vector<double> j3u(W, 0.0);
  if (h->has_j2) {
    TRY(jas_refresh(h));
    hipLaunchKernelGGL((k_jastrow_value<>), dim3((unsigned)W), dim3(64), 0, h->stream, h->S, h->js, (double*)h->b_ju.p);
    TRY(check_launch(h, "k_jastrow_value"));
    TRY(copy_in(h, ju.data(), h->b_ju.p, W * sizeof(double)));
  }
  if (h->has_j3) {
    TRY(j3_value_dev(h));
    TRY(copy_in(h, j3u.data(), h->b_j3u.p, W * sizeof(double)));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  for (long w = 0; w < W; ++w) lg[w] += ju[w] + j3u[w];
  if (sign) HIPCHK(hipMemcpy(sign, sg.data(), cf * W * sizeof(double), hipMemcpyDefault));
  if (logabs) HIPCHK(hipMemcpy(logabs, lg.data(), W * sizeof(double), hipMemcpyDefault));
  return 0;
}

extern "C" int pqa_wf_recompute(pqa_handle_t* h, const double* configs, int64_t W, double* sign, double* logabs) {
  h->dmc.old_valid = false;  // (the state pqa_dmc_continue refers to is gone)
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  TRY(ensure_walkers(h, W));
  h->jas_stale = false;
  TRY(copy_in(h, h->js.x, configs, (size_t)W * h->N * 3 * sizeof(double)));
  if (h->has_slater) TRY(slater_rebuild(h));
  if (h->has_j2) {
    hipLaunchKernelGGL((k_jastrow_recompute<>), dim3((unsigned)W), dim3(64), 0, h->stream, h->S, h->js);
    TRY(check_launch(h, "k_jastrow_recompute"));
  }
  return wf_value_host(h, sign, logabs);
}

extern "C" int pqa_wf_value(pqa_handle_t* h, double* sign, double* logabs) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("state not initialised (call recompute)");
  return wf_value_host(h, sign, logabs);
}

extern "C" int pqa_get_configs(pqa_handle_t* h, double* configs) { return pqa_jastrow_get_state(h, nullptr, nullptr, configs); }

// ---------------------------------------------------------------- branching on the device
// dst row w <- src row idx[w]; rows of `row` doubles.  grid = (W, ceil(row / 1024)), block = 256 (4 doubles per thread)
__global__ __launch_bounds__(256) void k_gather_rows(const double* __restrict__ src, double* __restrict__ dst, const int* __restrict__ idx,
                                                     long row) {
  const long w = blockIdx.x;
  const double* s = src + (size_t)idx[w] * row;
  double* d = dst + (size_t)w * row;
  for (long k = (long)blockIdx.y * 1024 + threadIdx.x; k < row && k < ((long)blockIdx.y + 1) * 1024; k += 256) d[k] = s[k];
}
static int gather_swap(pqa_handle* h, DevBuf& cur, DevBuf& alt, const int* d_idx, size_t row_doubles) {
  if (row_doubles == 0 || !cur.p) return 0;
  TRY(ensure(h, alt, (size_t)h->W * row_doubles * sizeof(double)));
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)h->W, (unsigned)((row_doubles + 1023) / 1024)), dim3(256), 0, h->stream,
                     (const double*)cur.p, (double*)alt.p, d_idx, (long)row_doubles);
  std::swap(cur, alt);
  return 0;
}
extern "C" int pqa_resample(pqa_handle_t* h, const int32_t* newinds) {
  h->dmc.old_valid = false;  // (the state pqa_dmc_continue refers to is gone)
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("state not initialised (call recompute)");
  if (!newinds) FAIL("pqa_resample: newinds must not be NULL");
  const long W = h->W;
  for (long w = 0; w < W; ++w)
    if (newinds[w] < 0 || newinds[w] >= W) FAIL("pqa_resample: index out of range");
  h->saved_valid = false;
  TRY(ensure(h, h->b_rsidx, (size_t)W * sizeof(int)));
  TRY(copy_in(h, h->b_rsidx.p, newinds, (size_t)W * sizeof(int)));
  const int* idx = (const int*)h->b_rsidx.p;
  for (const WalkerRow& r : walker_rows(h)) {
    if (!r.has) continue;
    if (!(r.jas_sum && h->jas_stale)) TRY(gather_swap(h, *r.cur, *r.alt, idx, r.row));
    if (r.ptr) *r.ptr = (double*)r.cur->p;
  }
  TRY(check_launch(h, "k_gather_rows"));
  HIPCHK(hipStreamSynchronize(h->stream));  // newinds may be freed by the caller
  return 0;
}

// ---------------------------------------------------------------- distributed branching (one walker exchange per block)
// dst row k <- src row idx[k] for k < n (k_gather_rows with a destination that is NOT one of the handle's buffers)
extern "C" int pqa_get_walkers(pqa_handle_t* h, const int32_t* idx, int64_t n, double* out) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("state not initialised (call recompute)");
  if (n <= 0) return 0;
  for (int64_t k = 0; k < n; ++k)
    if (idx[k] < 0 || idx[k] >= h->W) FAIL("pqa_get_walkers: index out of range");
  const size_t row = (size_t)h->N * 3;
  TRY(ensure(h, h->b_rsidx, (size_t)n * sizeof(int)));
  TRY(ensure(h, h->b_pts, (size_t)n * row * sizeof(double)));
  TRY(copy_in(h, h->b_rsidx.p, idx, (size_t)n * sizeof(int)));
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)n, (unsigned)((row + 1023) / 1024)), dim3(256), 0, h->stream, (const double*)h->js.x,
                     (double*)h->b_pts.p, (const int*)h->b_rsidx.p, (long)row);
  TRY(check_launch(h, "k_gather_rows"));
  return copy_out(h, out, h->b_pts.p, (size_t)n * row * sizeof(double));
}

// Wave-function state of walkers [w0, w0 + n) from their coordinates: the recompute pipeline run on a view of the state.
static int recompute_range(pqa_handle* h, long w0, long n) {
  if (n <= 0) return 0;
  const JastrowState js0 = h->js;
  const SlaterState st0 = h->st;
  const long W0 = h->W;
  for (const WalkerRow& r : walker_rows(h))
    if (r.has && r.ptr) *r.ptr += (size_t)w0 * r.row;
  h->W = n;
  int rc = 0;
  if (h->has_slater) rc = slater_rebuild(h);
  if (!rc && h->has_j2 && !h->jas_stale) {
    hipLaunchKernelGGL((k_jastrow_recompute<>), dim3((unsigned)n), dim3(64), 0, h->stream, h->S, h->js);
    rc = check_launch(h, "k_jastrow_recompute");
  }
  if (!rc && h->has_j3) {
    hipLaunchKernelGGL((k_j3_value<>), dim3((unsigned)n), dim3(64), lds_j3(h), h->stream, h->S, h->js, (double*)h->b_j3u.p + w0);
    rc = check_launch(h, "k_j3_value");
  }
  h->js = js0; h->st = st0; h->W = W0;
  return rc;
}

extern "C" int pqa_branch_exchange(pqa_handle_t* h, const int32_t* keep_src, int64_t nkeep, const double* recv_x, int64_t nrecv) {
  h->dmc.old_valid = false;  // (the state pqa_dmc_continue refers to is gone)
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("state not initialised (call recompute)");
  if (nkeep < 0 || nrecv < 0 || nkeep + nrecv != h->W) FAIL("pqa_branch_exchange: kept + received walkers must equal the resident count");
  std::vector<int32_t> idx((size_t)h->W, 0);
  for (int64_t k = 0; k < nkeep; ++k) idx[k] = keep_src[k];
  TRY(pqa_resample(h, idx.data()));  // received slots gather walker 0's state: overwritten below
  if (nrecv > 0) {
    TRY(copy_in(h, h->js.x + (size_t)nkeep * h->N * 3, recv_x, (size_t)nrecv * h->N * 3 * sizeof(double)));
    TRY(recompute_range(h, nkeep, nrecv));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// device-wide exclusive scan c[n] -> o[n+1]; marks[k] = o[k*Wm] for k = 0..n/Wm (pqa_dmc.hpp)
// ---------------------------------------------------------------- density-matrix sampling (pqa_dm.hpp)
extern "C" int pqa_dm_walk(pqa_handle_t* h, int slot, int spin, int64_t n, int nsamples, double tstep, double* pos, const double* gauss,
                           const double* unif, uint64_t seed, int nkeep, double* keep_pos, double* accept) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater) FAIL("handle has no orbital tables");
  if (slot < 0 || slot > 1 || spin < 0 || spin > 1) FAIL("pqa_dm_walk: slot and spin must be 0 or 1");
  if (n <= 0 || nsamples < 0 || nkeep < 0 || nkeep > nsamples) FAIL("pqa_dm_walk: bad sizes");
  if ((gauss == nullptr) != (unif == nullptr)) FAIL("pqa_dm_walk: give both tapes or neither");
  if (h->nmo[spin] == 0) FAIL("pqa_dm_walk: no orbitals for this spin");
  auto& d = h->dm[slot];
  const int nmo2 = h->nmo[spin];  // complex handles count [Re | Im] columns
  d.n = n; d.nkeep = nkeep; d.spin = spin;
  h->saved_valid = false;
  TRY(ensure(h, d.pos, (size_t)n * 3 * sizeof(double)));
  TRY(ensure(h, d.newpos, (size_t)n * 3 * sizeof(double)));
  TRY(ensure(h, d.row, (size_t)n * nmo2 * sizeof(double)));
  TRY(ensure(h, d.f, (size_t)n * sizeof(double)));
  TRY(ensure(h, d.keep_pos, (size_t)std::max(nkeep, 1) * n * 3 * sizeof(double)));
  TRY(ensure(h, d.keep_row, (size_t)std::max(nkeep, 1) * n * nmo2 * sizeof(double)));
  TRY(ensure(h, d.keep_f, (size_t)std::max(nkeep, 1) * n * sizeof(double)));
  TRY(ensure(h, h->b_motmp, (size_t)n * nmo2 * sizeof(double)));
  const int CH = 64;  // samples per tape upload
  if (gauss) {
    TRY(ensure(h, h->b_gauss, (size_t)CH * n * 3 * sizeof(double)));
    TRY(ensure(h, h->b_unif, (size_t)CH * n * sizeof(double)));
  }
  if (accept) TRY(ensure(h, h->dm_acc, (size_t)CH * n * sizeof(double)));
  TRY(copy_in(h, d.pos.p, pos, (size_t)n * 3 * sizeof(double)));
  const dim3 g256((unsigned)((n + 255) / 256));
  TRY(launch_orb(h, spin, plain_points((const double*)d.pos.p, n), n, 1, (double*)d.row.p));
  hipLaunchKernelGGL((k_dm_density<>), g256, dim3(256), 0, h->stream, (const double*)d.row.p, (long)n, nmo2, (double*)d.f.p);
  TRY(check_launch(h, "k_dm_density"));
  const double sq = sqrt(tstep);
  for (int s0 = 0; s0 < nsamples; s0 += CH) {
    const int ns = std::min(CH, nsamples - s0);
    if (gauss) {
      TRY(copy_in(h, h->b_gauss.p, gauss + (size_t)s0 * n * 3, (size_t)ns * n * 3 * sizeof(double)));
      TRY(copy_in(h, h->b_unif.p, unif + (size_t)s0 * n, (size_t)ns * n * sizeof(double)));
    }
    for (int k = 0; k < ns; ++k) {
      const int s = s0 + k, kk = s - (nsamples - nkeep);
      hipLaunchKernelGGL((k_dm_propose<>), g256, dim3(256), 0, h->stream, (const double*)d.pos.p,
                         gauss ? (const double*)h->b_gauss.p + (size_t)k * n * 3 : (const double*)nullptr, seed, (uint32_t)s, sq, (long)n,
                         (double*)d.newpos.p);
      TRY(launch_orb(h, spin, plain_points((const double*)d.newpos.p, n), n, 1, (double*)h->b_motmp.p));
      hipLaunchKernelGGL((k_dm_accept<>), dim3((unsigned)n), dim3(64), 0, h->stream, (double*)d.pos.p, (double*)d.row.p, (double*)d.f.p,
                         (const double*)d.newpos.p, (const double*)h->b_motmp.p,
                         unif ? (const double*)h->b_unif.p + (size_t)k * n : (const double*)nullptr, seed, (uint32_t)s, (long)n, nmo2,
                         accept ? (double*)h->dm_acc.p + (size_t)k * n : (double*)nullptr,
                         kk >= 0 ? (double*)d.keep_pos.p + (size_t)kk * n * 3 : (double*)nullptr,
                         kk >= 0 ? (double*)d.keep_row.p + (size_t)kk * n * nmo2 : (double*)nullptr,
                         kk >= 0 ? (double*)d.keep_f.p + (size_t)kk * n : (double*)nullptr);
    }
    TRY(check_launch(h, "k_dm_propose/k_dm_accept"));
    if (accept) TRY(copy_out(h, accept + (size_t)s0 * n, h->dm_acc.p, (size_t)ns * n * sizeof(double)));
  }
  TRY(copy_out(h, pos, d.pos.p, (size_t)n * 3 * sizeof(double)));
  if (keep_pos && nkeep > 0) TRY(copy_out(h, keep_pos, d.keep_pos.p, (size_t)nkeep * n * 3 * sizeof(double)));
  return 0;
}

extern "C" int pqa_dm_points(pqa_handle_t* h, int slot, int spin, const double* pts, int64_t npts) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater) FAIL("handle has no orbital tables");
  if (slot < 0 || slot > 1 || spin < 0 || spin > 1 || npts <= 0) FAIL("pqa_dm_points: bad arguments");
  auto& d = h->dm[slot];
  const int nmo2 = h->nmo[spin];
  h->saved_valid = false;
  TRY(ensure(h, h->b_pts, (size_t)npts * 3 * sizeof(double)));
  TRY(ensure(h, d.cfg, (size_t)npts * nmo2 * sizeof(double)));
  TRY(copy_in(h, h->b_pts.p, pts, (size_t)npts * 3 * sizeof(double)));
  d.ncfg = npts;
  return launch_orb(h, spin, plain_points((const double*)h->b_pts.p, npts), npts, 1, (double*)d.cfg.p);
}

int dm_prepare(pqa_handle* h, long nconf, long nval, int cx, int first, long nnorm_a, long nnorm_b) {
  if (first) { h->dm_nconf = nconf; h->dm_nval = nval; h->dm_cx = cx; }
  else if (h->dm_nconf != nconf || h->dm_nval != nval || h->dm_cx != cx) FAIL("density-matrix accumulation: shape changed since the first sweep");
  TRY(ensure(h, h->dm_val, (size_t)nconf * nval * (cx ? 2 : 1) * sizeof(double)));
  TRY(ensure(h, h->dm_norm[0], (size_t)nconf * std::max(nnorm_a, 1L) * sizeof(double)));
  TRY(ensure(h, h->dm_norm[1], (size_t)nconf * std::max(nnorm_b, 1L) * sizeof(double)));
  return 0;
}

extern "C" int pqa_obdm_accumulate(pqa_handle_t* h, int slot, int k, int64_t nconf, int nelec, const int32_t* assign, const double* ratio,
                                   int ratio_complex, int first) {
  HIPCHK(hipSetDevice(h->device));
  if (slot < 0 || slot > 1) FAIL("pqa_obdm_accumulate: slot must be 0 or 1");
  auto& d = h->dm[slot];
  if (k < 0 || k >= d.nkeep) FAIL("pqa_obdm_accumulate: sample was not kept by pqa_dm_walk");
  if (d.ncfg != nconf * nelec) FAIL("pqa_obdm_accumulate: pqa_dm_points was called with another number of points");
  const int oc = h->cplx ? 1 : 0, rc = ratio_complex ? 1 : 0, nmo2 = h->nmo[d.spin], norb = nmo2 / (oc ? 2 : 1);
  TRY(dm_prepare(h, nconf, (long)norb * norb, rc | oc, first, norb, 0));
  TRY(ensure(h, h->dm_assign[0], (size_t)nconf * sizeof(int)));
  TRY(ensure(h, h->dm_ratio, (size_t)nconf * nelec * (rc ? 2 : 1) * sizeof(double)));
  TRY(copy_in(h, h->dm_assign[0].p, assign, (size_t)nconf * sizeof(int)));
  TRY(copy_in(h, h->dm_ratio.p, ratio, (size_t)nconf * nelec * (rc ? 2 : 1) * sizeof(double)));
  hipLaunchKernelGGL((k_obdm_acc<>), dim3((unsigned)nconf), dim3(256), (size_t)2 * norb * sizeof(double), h->stream,
                     (const double*)d.keep_row.p + (size_t)k * d.n * nmo2, (const double*)d.keep_f.p + (size_t)k * d.n,
                     (const int*)h->dm_assign[0].p, (const double*)d.cfg.p, (const double*)h->dm_ratio.p, rc, oc, nelec, norb, first,
                     (double*)h->dm_val.p, (double*)h->dm_norm[0].p);
  return check_launch(h, "k_obdm_acc");
}

extern "C" int pqa_tbdm_accumulate(pqa_handle_t* h, int k, int64_t nconf, int nea, int neb, const int32_t* assign_a, const int32_t* assign_b,
                                   const double* ratio, int ratio_complex, const int32_t* ijkl, int ntuple, int first) {
  HIPCHK(hipSetDevice(h->device));
  auto& da = h->dm[0];
  auto& db = h->dm[1];
  if (k < 0 || k >= da.nkeep || k >= db.nkeep) FAIL("pqa_tbdm_accumulate: sample was not kept by pqa_dm_walk");
  if (da.ncfg != nconf * nea || db.ncfg != nconf * neb) FAIL("pqa_tbdm_accumulate: pqa_dm_points was called with other numbers of points");
  const int oc = h->cplx ? 1 : 0, rc = ratio_complex ? 1 : 0;
  const int na2 = h->nmo[da.spin], nb2 = h->nmo[db.spin], na = na2 / (oc ? 2 : 1), nb = nb2 / (oc ? 2 : 1);
  const size_t lds = (size_t)2 * ((size_t)nea * nb + (size_t)na * nb) * sizeof(double);
  if (lds > 64 * 1024) FAIL("pqa_tbdm_accumulate: orbital basis too large for the per-walker LDS tiles");
  TRY(dm_prepare(h, nconf, ntuple, rc | oc, first, na, nb));
  TRY(ensure(h, h->dm_assign[0], (size_t)nconf * sizeof(int)));
  TRY(ensure(h, h->dm_assign[1], (size_t)nconf * sizeof(int)));
  TRY(ensure(h, h->dm_ratio, (size_t)nconf * nea * neb * (rc ? 2 : 1) * sizeof(double)));
  TRY(ensure(h, h->dm_ijkl, (size_t)4 * ntuple * sizeof(int)));
  TRY(copy_in(h, h->dm_assign[0].p, assign_a, (size_t)nconf * sizeof(int)));
  TRY(copy_in(h, h->dm_assign[1].p, assign_b, (size_t)nconf * sizeof(int)));
  TRY(copy_in(h, h->dm_ratio.p, ratio, (size_t)nconf * nea * neb * (rc ? 2 : 1) * sizeof(double)));
  TRY(copy_in(h, h->dm_ijkl.p, ijkl, (size_t)4 * ntuple * sizeof(int)));
  hipLaunchKernelGGL((k_tbdm_acc<>), dim3((unsigned)nconf), dim3(256), lds, h->stream,
                     (const double*)da.keep_row.p + (size_t)k * da.n * na2, (const double*)da.keep_f.p + (size_t)k * da.n,
                     (const double*)db.keep_row.p + (size_t)k * db.n * nb2, (const double*)db.keep_f.p + (size_t)k * db.n,
                     (const int*)h->dm_assign[0].p, (const int*)h->dm_assign[1].p, (const double*)da.cfg.p, (const double*)db.cfg.p,
                     (const double*)h->dm_ratio.p, rc, oc, nea, neb, na, nb, (const int*)h->dm_ijkl.p, ntuple, first,
                     (double*)h->dm_val.p, (double*)h->dm_norm[0].p, (double*)h->dm_norm[1].p);
  return check_launch(h, "k_tbdm_acc");
}

// which: 0 value (dm_nval entries per configuration, interleaved complex if any input was), 1 norm (first / a), 2 norm b of
// `ncol` entries; mean != 0: average over the configurations on the device
extern "C" int pqa_dm_fetch(pqa_handle_t* h, int which, int ncol, double scale, int mean, double* out) {
  HIPCHK(hipSetDevice(h->device));
  if (h->dm_nconf <= 0) FAIL("pqa_dm_fetch: nothing accumulated");
  const double* src;
  long cols;
  if (which == 0) { src = (const double*)h->dm_val.p; cols = h->dm_nval * (h->dm_cx ? 2 : 1); }
  else if (which == 1 || which == 2) { src = (const double*)h->dm_norm[which - 1].p; cols = ncol; }
  else FAIL("pqa_dm_fetch: which must be 0, 1 or 2");
  if (which == 0 && ncol != cols) FAIL("pqa_dm_fetch: ncol does not match the accumulated value");
  const long nout = mean ? cols : h->dm_nconf * cols;
  TRY(ensure(h, h->dm_tmp, (size_t)nout * sizeof(double)));
  if (mean) hipLaunchKernelGGL((k_col_means<>), dim3((unsigned)cols), dim3(256), 0, h->stream, src, h->dm_nconf, cols, scale, (double*)h->dm_tmp.p);
  else hipLaunchKernelGGL((k_scale_copy<>), dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, h->stream, src, nout, scale, (double*)h->dm_tmp.p);
  TRY(check_launch(h, "pqa_dm_fetch"));
  return copy_out(h, out, h->dm_tmp.p, (size_t)nout * sizeof(double));
}

extern "C" int pqa_gram(pqa_handle_t* h, int64_t n, int P, int Q, const double* A, const double* B, double* C) {
  HIPCHK(hipSetDevice(h->device));
  if (n <= 0 || P <= 0 || Q <= 0) FAIL("pqa_gram: bad sizes");
  const int tiles = ((P + 15) / 16) * ((Q + 15) / 16);
  int nslice = (int)std::min<long>(std::max<long>(1, 1024 / tiles), std::max<long>(1, n / 64));
  DevBuf &a = h->b_pts, &b = h->b_out, &part = h->dm_tmp, &c = h->dm_acc;
  TRY(ensure(h, a, (size_t)n * P * sizeof(double)));
  TRY(ensure(h, b, (size_t)n * Q * sizeof(double)));
  TRY(ensure(h, part, (size_t)nslice * P * Q * sizeof(double)));
  TRY(ensure(h, c, (size_t)P * Q * sizeof(double)));
  TRY(copy_in(h, a.p, A, (size_t)n * P * sizeof(double)));
  TRY(copy_in(h, b.p, B, (size_t)n * Q * sizeof(double)));
  hipLaunchKernelGGL((k_gram_mfma<>), dim3((unsigned)((P + 15) / 16), (unsigned)((Q + 15) / 16), (unsigned)nslice), dim3(64), 0, h->stream,
                     (const double*)a.p, (const double*)b.p, (long)n, P, Q, nslice, (double*)part.p);
  hipLaunchKernelGGL((k_gram_reduce<>), dim3((unsigned)(((long)P * Q + 255) / 256)), dim3(256), 0, h->stream, (const double*)part.p, (long)P * Q,
                     nslice, (double*)c.p);
  TRY(check_launch(h, "k_gram_mfma"));
  return copy_out(h, C, c.p, (size_t)P * Q * sizeof(double));
}

// The standard normals and Metropolis uniforms the fused sweeps draw for (seed, step): gauss (N,W,3), unif (N,W) for
// walkers 0..W-1 (the streams are keyed by walker index, so any prefix of an ensemble can be asked for).
extern "C" int pqa_philox_tapes(pqa_handle_t* h, uint64_t seed, int step, int64_t W, double* gauss, double* unif) {
  HIPCHK(hipSetDevice(h->device));
  if (W <= 0 || step < 0 || !gauss || !unif) FAIL("pqa_philox_tapes: bad arguments");
  const size_t NW = (size_t)h->N * W;
  TRY(ensure(h, h->b_gauss, NW * 3 * sizeof(double)));
  TRY(ensure(h, h->b_unif, NW * sizeof(double)));
  hipLaunchKernelGGL((k_tile_draws<>), dim3((unsigned)((NW + 255) / 256)), dim3(256), 0, h->stream, seed, (uint32_t)step, h->N, (long)W,
                     (double*)h->b_gauss.p, (double*)h->b_unif.p);
  TRY(check_launch(h, "k_tile_draws"));
  TRY(copy_in(h, gauss, h->b_gauss.p, NW * 3 * sizeof(double)));
  return copy_out(h, unif, h->b_unif.p, NW * sizeof(double));
}

// out[c][w] = the uniform of Philox(seed; walker w, counter c, stream, step) — what ecp_pass / k_tm_count / k_tm_walker draw
static __global__ __launch_bounds__(256) void k_uniform_plane(uint64_t seed, uint32_t stream, uint32_t step, long ncount, long W, double* __restrict__ out) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ncount * W) return;
  const long c = idx / W, w = idx - c * W;
  const Philox p = philox(seed, (uint32_t)w, (uint32_t)c, stream, step);
  out[idx] = u01(p.c[0], p.c[1]);
}
// out[e][w][j] = the uniform of Philox(seed; walker w, counter e nsr + j, stream, step) — the selection draws of k_ecpb_fill
static __global__ __launch_bounds__(256) void k_uniform_sel(uint64_t seed, uint32_t stream, uint32_t step, int nelec, long W, int nsr, double* __restrict__ out) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)nelec * W * nsr) return;
  const int j = (int)(idx % nsr);
  const long ew = idx / nsr, e = ew / W, w = ew - e * W;
  const Philox p = philox(seed, (uint32_t)w, (uint32_t)(e * nsr + j), stream, step);
  out[idx] = u01(p.c[0], p.c[1]);
}
extern "C" int pqa_philox_dmc_tapes(pqa_handle_t* h, uint64_t seed, int nsteps, int64_t W, pqa_dmc_tapes_t* out) {
  HIPCHK(hipSetDevice(h->device));
  if (W <= 0 || nsteps <= 0 || !out || !out->gauss || !out->unif) FAIL("pqa_philox_dmc_tapes: bad arguments");
  const int N = h->N, necp = h->necp;
  const DmcDraws d = dmc_draws(h);  // (the layout of ecp_unif / tm_unif, and whether they exist)
  const size_t NW = (size_t)N * W, nrot = d.nrot;
  if (necp > 0 && (!out->ecp_rot || (d.nu > 0 && !out->ecp_unif))) FAIL("pqa_philox_dmc_tapes: ECP systems need ecp_rot and ecp_unif");
  const bool tm = necp > 0 && out->tm_rot && (d.nu == 0 || out->tm_unif) && out->tm_u1 && out->tm_u2;
  TRY(ensure(h, h->b_gauss, NW * 3 * sizeof(double)));
  TRY(ensure(h, h->b_unif, NW * std::max(d.nu, 1) * sizeof(double)));
  TRY(ensure(h, h->b_rot, nrot * 9 * sizeof(double)));
  auto plane = [&](uint32_t stream, uint32_t step, size_t ncount, const double* dst) -> int {
    hipLaunchKernelGGL(k_uniform_plane, dim3((unsigned)((ncount * W + 255) / 256)), dim3(256), 0, h->stream, seed, stream, step, (long)ncount, (long)W,
                       (double*)h->b_unif.p);
    TRY(check_launch(h, "k_uniform_plane"));
    return copy_out(h, const_cast<double*>(dst), h->b_unif.p, ncount * W * sizeof(double));
  };
  auto sel = [&](uint32_t stream, uint32_t step, const double* dst) -> int {
    hipLaunchKernelGGL(k_uniform_sel, dim3((unsigned)((NW * d.nsr + 255) / 256)), dim3(256), 0, h->stream, seed, stream, step, N, (long)W, d.nsr, (double*)h->b_unif.p);
    TRY(check_launch(h, "k_uniform_sel"));
    return copy_out(h, const_cast<double*>(dst), h->b_unif.p, NW * d.nsr * sizeof(double));
  };
  auto rots = [&](uint64_t sd, uint32_t step, const double* dst) -> int {
    hipLaunchKernelGGL((k_gen_rot<>), dim3((unsigned)((nrot + 63) / 64)), dim3(64), 0, h->stream, (int)nrot, sd, step, (double*)h->b_rot.p);
    TRY(check_launch(h, "k_gen_rot"));
    return copy_out(h, const_cast<double*>(dst), h->b_rot.p, nrot * 9 * sizeof(double));
  };
  for (int i = 0; i <= nsteps; ++i) {
    if (necp > 0) {  // energy evaluation i (0: the starting configuration; energy_dev's draws)
      TRY(rots(seed, (uint32_t)i, out->ecp_rot + (size_t)i * nrot * 9));
      if (!d.batched) TRY(plane(PQA_STREAM_ECPMASK, (uint32_t)i, nrot, out->ecp_unif + (size_t)i * NW * d.nu));
      else if (d.selu) TRY(sel(PQA_STREAM_ECPSEL, (uint32_t)i, out->ecp_unif + (size_t)i * NW * d.nu));
    }
    if (i == nsteps) break;
    if (tm) {
      TRY(rots(seed ^ 0x9E3779B97F4A7C15ull, (uint32_t)i, out->tm_rot + (size_t)i * nrot * 9));
      if (!d.batched) TRY(plane(PQA_STREAM_TMMASK, (uint32_t)i, nrot, out->tm_unif + (size_t)i * NW * d.nu));
      else if (d.selu) TRY(sel(PQA_STREAM_TMSEL, (uint32_t)i, out->tm_unif + (size_t)i * NW * d.nu));
      TRY(plane(PQA_STREAM_TM_U1, (uint32_t)i, (size_t)N, out->tm_u1 + (size_t)i * NW));
      TRY(plane(PQA_STREAM_TM_U2, (uint32_t)i, (size_t)N, out->tm_u2 + (size_t)i * NW));
    }
    hipLaunchKernelGGL((k_tile_draws<>), dim3((unsigned)((NW + 255) / 256)), dim3(256), 0, h->stream, seed, (uint32_t)i, N, (long)W,
                       (double*)h->b_gauss.p, (double*)h->b_unif.p);
    TRY(check_launch(h, "k_tile_draws"));
    TRY(copy_in(h, const_cast<double*>(out->gauss) + (size_t)i * NW * 3, h->b_gauss.p, NW * 3 * sizeof(double)));
    TRY(copy_out(h, const_cast<double*>(out->unif) + (size_t)i * NW, h->b_unif.p, NW * sizeof(double)));
  }
  return 0;
}

extern "C" int pqa_sync(pqa_handle_t* h) {
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
extern "C" int pqa_timer_start(pqa_handle_t* h) {
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  return 0;
}
extern "C" int pqa_timer_stop(pqa_handle_t* h, double* elapsed_ms) {
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  HIPCHK(hipEventSynchronize(h->ev1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *elapsed_ms = ms;
  return 0;
}
extern "C" int pqa_profile_enable(pqa_handle_t* h, int enable) {
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->profile = enable != 0;
  for (ProfSet* p : {&h->prof_orb, &h->prof_commit, &h->prof_part}) { p->used = 0; p->launches = 0; p->ms = 0.0; }
  h->prof_pc = 0.0;
  return 0;
}
extern "C" int pqa_profile_query(pqa_handle_t* h, int64_t* launches, double* total_ms, double* point_comps) {
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  TRY(prof_drain(h, h->prof_orb));
  if (launches) *launches = h->prof_orb.launches;
  if (total_ms) *total_ms = h->prof_orb.ms;
  if (point_comps) *point_comps = h->prof_pc;
  return 0;
}
extern "C" int pqa_profile_query_commit(pqa_handle_t* h, int64_t* launches, double* total_ms) {
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  TRY(prof_drain(h, h->prof_commit));
  if (launches) *launches = h->prof_commit.launches;
  if (total_ms) *total_ms = h->prof_commit.ms;
  return 0;
}
extern "C" int pqa_profile_query_part(pqa_handle_t* h, int64_t* launches, double* total_ms, int* groups) {
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  TRY(prof_drain(h, h->prof_part));
  if (launches) *launches = h->prof_part.launches;
  if (total_ms) *total_ms = h->prof_part.ms;
  if (groups) *groups = lw_geometry(h, h->W).Gm;
  return 0;
}
extern "C" int pqa_set_ecp_naip(pqa_handle_t* h, int32_t naip) {
  HIPCHK(hipSetDevice(h->device));
  if (naip != 0 && ecp_quadrature_offset(naip) < 0) FAIL("naip must be one of 6, 12, 18, 26, 32, 50 (eval_ecp.py:266-267), or 0 for the per-atom default");
  if (h->necp == 0) { h->ecp_naip = naip; return 0; }
  std::vector<int> na((size_t)h->necp), qo((size_t)h->necp);
  for (int k = 0; k < h->necp; ++k) {
    na[k] = naip ? naip : (h->ecp_nch[k] <= 2 ? 6 : 12);
    qo[k] = ecp_quadrature_offset(na[k]);
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  h->en.hint_valid = false; h->en.last_dev[0] = h->en.last_dev[1] = nullptr;  // (another rule: other point totals)
  if (h->en.last_points < 0) h->en.last_points = 0;
  h->S.ecp_naip_max = 0;
  for (int k = 0; k < h->necp; ++k) h->S.ecp_naip_max = std::max(h->S.ecp_naip_max, na[k]);
  HIPCHK(hipMemcpy(h->d_ecp_naip, na.data(), na.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d_ecp_qoff, qo.data(), qo.size() * sizeof(int), hipMemcpyHostToDevice));
  h->ecp_naip = naip;
  return 0;
}
extern "C" int pqa_last_ecp_points(pqa_handle_t* h, int64_t* npoints) {
  if (h->en.last_points < 0 && h->en.last_dev[0]) {  // the last evaluation left its totals on the device (pqa_energy.hip)
    HIPCHK(hipSetDevice(h->device));
    long t[2];
    TRY(copy_in(h, &t[0], h->en.last_dev[0], sizeof(long)));
    TRY(copy_out(h, &t[1], h->en.last_dev[1], sizeof(long)));
    h->en.last_points = t[0] + t[1];
  }
  *npoints = h->en.last_points;
  return 0;
}
