// Host side of xm_espirit_eig (include/xmris_hip.h); the kernel is in xm_espirit.h.
#include "xm_host.h"
#include "xm_espirit.h"

#include <string>

static int esp_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "espirit_eig: " + msg); }

namespace {
XmResidency g_esp_res;
}

extern "C" int xm_espirit_eig(const void* h, void* maps, double* values, int32_t* status, int64_t n_vox, int n_coils,
                              int n_maps, int phase_ref, double crop, void* stream) {
  if (n_coils < 1 || n_coils > XM_ESP_MAXC) return esp_fail("n_coils must be in 1 ... 64");
  if (n_maps < 1 || n_maps > 2 || n_maps > n_coils) return esp_fail("n_maps must be in 1 ... min(2, n_coils)");
  if (n_vox < 1 || n_vox > (1LL << 31) - 1) return esp_fail("n_vox must be in 1 ... 2^31 - 1");
  if (phase_ref < 0 || phase_ref >= n_coils) return esp_fail("phase_ref must be in 0 ... n_coils - 1");
  if (!std::isfinite(crop)) return esp_fail("crop must be finite");
  if (!h || !maps || !values || !status) return esp_fail("null pointer");
  if ((reinterpret_cast<size_t>(h) & 15) || (reinterpret_cast<size_t>(maps) & 15) || (reinterpret_cast<size_t>(values) & 7) ||
      (reinterpret_cast<size_t>(status) & 3))
    return esp_fail("a pointer is not aligned to its element size");
  const void* outs[3] = {maps, values, status};
  for (int i = 0; i < 3; ++i) {
    if (outs[i] == h) return esp_fail("an output aliases the input");
    for (int j = 0; j < i; ++j)
      if (outs[i] == outs[j]) return esp_fail("an output aliases another output");
  }

  EspArgs A{};
  A.h = static_cast<const double*>(h);
  A.maps = static_cast<double*>(maps);
  A.values = values;
  A.status = status;
  A.V = n_vox;
  A.C = n_coils;
  A.M = n_maps;
  A.phase_ref = phase_ref;
  A.crop = crop;

  DeviceGuard guard(h);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = esp_lds_bytes(n_coils);
  int resident = 0;
  if (const int rc = xm_resident_blocks(g_esp_res, k_espirit_eig, XM_ESP_NT, lds, &resident, st)) return rc;
  const long long blocks = n_vox < resident ? n_vox : resident;
  xm_note_kernel("k_espirit_eig", nullptr, "c128", n_coils, n_maps);  // <coils, maps>
  hipLaunchKernelGGL(k_espirit_eig, dim3((unsigned)blocks), dim3(XM_ESP_NT), lds, st, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}
