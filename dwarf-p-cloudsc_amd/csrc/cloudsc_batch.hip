// cloudsc_batch.hip -- the batched step: many caller-owned field sets of one shape in one KCACHE launch, each set
// under its own parameter set (include/cloudsc_amd.h).
//
// A batch owns two device allocations: the table -- one kernel-argument struct per set, built exactly as
// cloudsc_gpu_run_outputs builds the one it passes by value -- and, with per-set parameters, one parameter block per
// set, each entry's `par` pointing at its own.  Without them every `par` is the device's default block, whose
// address outlives a later cloudsc_gpu_init.  Both are uploaded once, at creation; a run is one launch of
// kcache_batch_entry (cloudsc_gpu.hip), which takes the member index from the grid's y dimension.
//
// Every argument rule is checked before the first HIP call, so an argument error is CLOUDSC_EINVAL on a machine
// without a GPU too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "cloudsc_amd.h"
#include "cloudsc_internal.h"

using namespace cloudsc_impl;

struct cloudsc_batch {
  int device = -1;
  int precision = 0, outputs = 0, nsets = 0, ngptot = 0, nproma = 0, klev = 0;
  bool own_params = false;    // per-set parameter blocks (else: the device's default set, looked up at each run)
  bool aer = false;           // own_params: LAERICESED || LAERICEAUTO of every set
  bool aer_members = false;   // picrit_aer, pre_ice, pnice are set in every set
  void* table = nullptr;      // device: nsets entries, batch_entry_stride() apart
  void* params = nullptr;     // device: nsets parameter blocks (own_params)
};

namespace {

size_t param_block_stride() { return (param_block_bytes() + 255) & ~(size_t)255; }

bool is_written(int member, int outputs) {
  const int dir = kFieldTable[member].dir;
  return (dir == CLOUDSC_FD_OUT || dir == CLOUDSC_FD_INOUT) && output_selected(member, outputs);
}

// The aliasing rule, pointer equality only: a member the step writes (a selected output, plude) equals no other
// non-NULL member of any set.  Sorted, so that the cap of 65535 sets costs n log n.
bool aliasing_ok(const cloudsc_fields_t* sets, int nsets, int outputs) {
  struct Ref { const void* p; bool written; };
  std::vector<Ref> refs;
  refs.reserve((size_t)nsets * kNumFields);
  for (int i = 0; i < nsets; i++) {
    const void* const* p = (const void* const*)&sets[i];
    for (int m = 0; m < kNumFields; m++)
      if (p[m]) refs.push_back({p[m], is_written(m, outputs)});
  }
  std::sort(refs.begin(), refs.end(), [](const Ref& a, const Ref& b) { return std::less<const void*>()(a.p, b.p); });
  for (size_t i = 0; i + 1 < refs.size(); i++)
    if (refs[i].p == refs[i + 1].p && (refs[i].written || refs[i + 1].written)) return false;
  return true;
}

// every rule of cloudsc_batch_create that needs no device; *aer_members: the three aerosol inputs are set (in every set)
int check_create_args(cloudsc_batch_t** batch, int precision, int outputs, int nsets, int ngptot, int nproma, int klev,
                      const cloudsc_fields_t* sets, const cloudsc_params_t* params, bool* aer_members, bool* aer) {
  if (!batch || !sets) return CLOUDSC_EINVAL;
  if (nsets < 1 || nsets > CLOUDSC_BATCH_MAX_SETS) return CLOUDSC_EINVAL;
  if (!outputs_known(outputs)) return CLOUDSC_EINVAL;
  // the per-set rules of cloudsc_gpu_run_outputs with KCACHE: precision, 1 <= nproma <= 256, ngptot >= 1, klev >= 2
  int rc = validate_shape_args(precision, CLOUDSC_VARIANT_KCACHE, ngptot, nproma, klev);
  if (rc) return rc;
  StepForm form;
  form.outputs = outputs;
  // the aerosol inputs the kernels read: each of them set in every set or in none
  const auto aer_bits = [](const cloudsc_fields_t& f) {
    return (f.picrit_aer ? 1 : 0) | (f.pre_ice ? 2 : 0) | (f.pnice ? 4 : 0);
  };
  for (int i = 0; i < nsets; i++) {
    if (!fields_complete(&sets[i], form)) return CLOUDSC_EINVAL;
    if (aer_bits(sets[i]) != aer_bits(sets[0])) return CLOUDSC_EINVAL;
  }
  *aer_members = aer_bits(sets[0]) == 7;
  *aer = false;
  if (params) {
    for (int i = 0; i < nsets; i++) {
      if ((rc = check_params(&params[i]))) return rc;
      const bool a = params[i].laericesed || params[i].laericeauto;
      if (i == 0) *aer = a;
      else if (a != *aer) return CLOUDSC_EINVAL;   // one kernel per batch: with the aerosol inputs or without
    }
    if (*aer && !*aer_members) return CLOUDSC_EINVAL;
  }
  if (!aliasing_ok(sets, nsets, outputs)) return CLOUDSC_EINVAL;
  return CLOUDSC_OK;
}

void batch_free(cloudsc_batch_t* b) {
  if (b->table) (void)hipFree(b->table);
  if (b->params) (void)hipFree(b->params);
  delete b;
}

}  // namespace

extern "C" {

int cloudsc_batch_create(cloudsc_batch_t** batch, int device, int precision, int outputs, int nsets, int ngptot,
                         int nproma, int klev, const cloudsc_fields_t* sets, const cloudsc_params_t* params) {
  bool aer_members = false, aer = false;
  int rc = check_create_args(batch, precision, outputs, nsets, ngptot, nproma, klev, sets, params, &aer_members, &aer);
  if (rc) return rc;
  *batch = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n || device >= kMaxDevices) return CLOUDSC_ENODEV;
  const ParamSet* dflt = nullptr;
  if (!params) {
    dflt = device_default_params(device);
    if (!dflt || !dflt->dev) return CLOUDSC_ENOINIT;
    if (dflt->aer && !aer_members) return CLOUDSC_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  cloudsc_batch_t* b = new (std::nothrow) cloudsc_batch_t;
  if (!b) return CLOUDSC_ENOMEM;
  b->device = device;
  b->precision = precision; b->outputs = outputs; b->nsets = nsets;
  b->ngptot = ngptot; b->nproma = nproma; b->klev = klev;
  b->own_params = params != nullptr;
  b->aer = aer;
  b->aer_members = aer_members;
  const size_t es = batch_entry_stride(), ps = param_block_stride();
  hipError_t e = hipMalloc(&b->table, es * (size_t)nsets);
  if (e == hipSuccess && params) e = hipMalloc(&b->params, ps * (size_t)nsets);
  if (e != hipSuccess) {
    hip_fail(e, "hipMalloc(batch)");
    batch_free(b);
    return CLOUDSC_ENOMEM;
  }
  std::vector<char> table(es * (size_t)nsets, 0), blocks(params ? ps * (size_t)nsets : 0, 0);
  for (int i = 0; i < nsets; i++) {
    const void* block = params ? (const char*)b->params + ps * (size_t)i : dflt->dev;
    if (params) param_block_fill(blocks.data() + ps * (size_t)i, params[i]);
    batch_make_entry(precision, table.data() + es * (size_t)i, &sets[i], ngptot, nproma, klev, block);
  }
  // on the null stream and waited for, as a parameter set's upload: the launches run on streams that do not
  // wait for the null stream, and a copy from pageable memory may return before the bytes have arrived
  e = hipMemcpyAsync(b->table, table.data(), table.size(), hipMemcpyHostToDevice, nullptr);
  if (e == hipSuccess && params)
    e = hipMemcpyAsync(b->params, blocks.data(), blocks.size(), hipMemcpyHostToDevice, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    batch_free(b);
    return hip_fail(e, "upload(batch)");
  }
  *batch = b;
  return CLOUDSC_OK;
}

int cloudsc_gpu_run_batch(cloudsc_batch_t* batch, void* stream, int variant) {
  // the variant first: KCACHE alone, no option bits -- KSEG's workspace and hand-off records are per set
  if (!batch || variant != CLOUDSC_VARIANT_KCACHE) return CLOUDSC_EINVAL;
  bool aer = batch->aer;
  if (!batch->own_params) {   // the device's set as it is now (its block's address does not change)
    const ParamSet* dflt = device_default_params(batch->device);
    if (!dflt || !dflt->dev) return CLOUDSC_ENOINIT;
    aer = dflt->aer;
    if (aer && !batch->aer_members) return CLOUDSC_EINVAL;
  }
  HIPCHK(hipSetDevice(batch->device));
  return launch_kcache_batch(stream, BatchLaunch{batch->precision, batch->outputs, batch->nsets, batch->ngptot,
                                                 batch->nproma, batch->klev, aer, batch->table});
}

int cloudsc_batch_nsets(const cloudsc_batch_t* batch) { return batch ? batch->nsets : CLOUDSC_EINVAL; }

int cloudsc_batch_destroy(cloudsc_batch_t* batch) {
  if (!batch) return CLOUDSC_OK;
  HIPCHK(hipSetDevice(batch->device));
  HIPCHK(hipDeviceSynchronize());   // a launch may still read the table
  batch_free(batch);
  return CLOUDSC_OK;
}

int cloudsc_batch_launch_geometry(int precision, int nsets, int ngptot, int nproma, int klev, int laer,
                                  cloudsc_launch_geometry_t* out) {
  if (nsets < 1 || nsets > CLOUDSC_BATCH_MAX_SETS) return CLOUDSC_EINVAL;
  const int rc = cloudsc_gpu_launch_geometry(precision, CLOUDSC_VARIANT_KCACHE, ngptot, nproma, klev, laer, out);
  if (rc) return rc;
  if ((long long)out->workgroups * nsets > 0x7fffffffLL) return CLOUDSC_EINVAL;
  out->units *= nsets;
  out->workgroups *= nsets;
  return CLOUDSC_OK;
}

}  // extern "C"
