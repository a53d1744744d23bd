// vame_pack.hip -- vame_pack_records (include/vame.h): a batch's result
// records into the compact wire form, one kernel over a segment table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vame.h"
#include "vame_ctx.h"
#include "vame_tables.h"

using namespace vame;

// Compact wire form (shard.pack's specification): thread i of segment
// blockIdx.y moves record i -- its cost as int32, its 2 * ncp CPMV components
// -- and flags a record the form cannot hold (cost outside [0, 2^31), a 2-CP
// LB other than (0, 0)).
__global__ __launch_bounds__(256) void pack_records_kernel(const PackSeg* segs, int32_t* slab, int32_t* bad) {
  const PackSeg sg = segs[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= sg.n) return;
  const long long c = sg.cost[i];
  const int32_t* r = sg.cpmv + (size_t)i * 7;
  int flag = (c < 0 || c >= (1ll << 31)) ? 1 : 0;
  slab[sg.off + i] = (int32_t)c;
  int32_t* d = slab + sg.off + sg.n + (size_t)i * 2 * sg.ncp;
  if (sg.ncp == 2) {
    d[0] = r[1]; d[1] = r[2]; d[2] = r[3]; d[3] = r[4];
    flag |= (r[5] | r[6]) != 0;
  } else {
    d[0] = r[1]; d[1] = r[2]; d[2] = r[3]; d[3] = r[4]; d[4] = r[5]; d[5] = r[6];
  }
  if (__builtin_amdgcn_ballot_w64(flag != 0) && flag) atomicOr(bad, 1);
}

extern "C" int vame_pack_records(vame_ctx* c, const vame_poc_job* jobs, int njobs, int mode_mask, int32_t* slab,
                                 long long words, int32_t* bad, void* stream) {
  if (!c || !jobs || njobs < 0 || !slab || !bad || words < 0) return VAME_E_INVALID;
  if (!(mode_mask & VAME_MODE_2CP) || (mode_mask & ~15)) return VAME_E_INVALID;
  const int preds = vame_pred_mask(mode_mask);
  DeviceGuard guard(c->device);
  VAME_HIP(guard.err);
  // the previous pack kernel read the device table (and the upload the host
  // one): both are rewritten below
  if (c->packEv) VAME_HIP(hipEventSynchronize(c->packEv));
  std::vector<PackSeg>& segs = c->packSegs;
  segs.clear();
  long long off = 0;
  int maxn = 0;
  for (int j = 0; j < njobs; j++) {
    const vame_poc_job& jb = jobs[j];
    if (!jb.out || jb.nrefs < 1 || jb.nrefs > 4) return VAME_E_INVALID;
    for (int r = 0; r < jb.nrefs; r++)
      for (int m = 0; m < 4; m++) {
        if (!((preds >> m) & 1)) continue;
        if (!jb.out->cost[r][m] || !jb.out->cpmvs[r][m]) return VAME_E_INVALID;
        PackSeg sg;
        sg.cost = jb.out->cost[r][m];
        sg.cpmv = reinterpret_cast<const int32_t*>(jb.out->cpmvs[r][m]);
        sg.n = c->nCtus * ((m >> 1) ? kHalfCusPerCtu : kFullCusPerCtu);
        sg.ncp = (m & 1) ? 3 : 2;
        sg.off = off;
        off += (long long)sg.n * (1 + 2 * sg.ncp);
        maxn = std::max(maxn, sg.n);
        segs.push_back(sg);
      }
  }
  if (off > words) return VAME_E_INVALID;
  hipStream_t s = (hipStream_t)stream;
  if (!c->packEv) VAME_HIP(hipEventCreateWithFlags(&c->packEv, hipEventDisableTiming));
  if (segs.size() > c->dPackCap) {
    if (c->dPackSegs) VAME_HIP(hipFree(c->dPackSegs));
    c->dPackSegs = nullptr;
    c->dPackCap = 0;
    VAME_HIP(hipMalloc(&c->dPackSegs, segs.size() * sizeof(PackSeg)));
    c->dPackCap = segs.size();
  }
  if (!segs.empty()) {
    VAME_HIP(hipMemcpyAsync(c->dPackSegs, segs.data(), segs.size() * sizeof(PackSeg), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(pack_records_kernel, dim3((maxn + 255) / 256, (unsigned)segs.size()), dim3(256), 0, s,
                       c->dPackSegs, slab, bad);
    VAME_HIP(hipGetLastError());
    VAME_HIP(hipEventRecord(c->packEv, s));  // after the kernel: the next call waits for its table reads
  }
  if (words > off) VAME_HIP(hipMemsetAsync(slab + off, 0, (size_t)(words - off) * sizeof(int32_t), s));
  return VAME_OK;
}
