// vame_main.cpp -- `vame`, the drop-in for the reference's ./main
// (main.cpp:53-1122): same flags and defaults, same CSV inputs, same per-CU
// decision logs (byte for byte), same stdout report keys -- with the affine ME
// running as HIP kernels on MI355X through libvame.so (include/vame.h).
//
//   vame -f N -s WxH -q QP -o orig.csv -r recon.csv [-l prefix]
//        [--ExtraGradientIter K] [--DeviceIndex D]
//   extensions: --gpus G      frame-shard POCs over G devices (D .. D+G-1),
//                             one host thread + context per device
//               --devices L   explicit device list (e.g. 0,1,2,3)
//               --modes all|2cp   all four PREDs (default) or the 2-CP ones
//               --align both|full|half   both alignments (default) or one
//               --per-launch  one launch per (refIdx, PRED) as the reference
//                             does (per-PRED kernel times); default = fused
//                             per-POC launch (vame_affine_me_poc)
//               --threads T   host threads for CSV parsing / log formatting
//               --prof        PROF on (the reference hard-disables it,
//                             affine.cl:168; vame_set_prof)
//
// Differences to the reference host, all deliberate:
//  * the 4-slot reference ring (main.cpp:591-707) is label bookkeeping only:
//    every recon frame is uploaded once and refIdx r points at the frame the
//    ring holds (vame_ref_list), so the ring's D2D copies disappear;
//  * it keeps 4 slots for any N (the reference allocates N_FRAMES ring buffers
//    into a 4-entry array, main.cpp:343-349);
//  * results are copied back asynchronously and the logs are formatted on the
//    host while the GPU runs the next POC; stdout keeps the reference's order;
//  * the OpenCL platform/device listing becomes a HIP device listing, and the
//    per-PRED START/FINISH EXEC timestamps are not printed (PREDs are fused);
//  * in the default fused mode one launch computes all four PREDs, so the
//    reference's per-PRED *_EXEC keys carry the fused kernel time apportioned
//    by each PRED's algorithmic work (sub-block predictions of its in-frame
//    CUs, n_pred = 6 for 2 CP / 5 for 3 CP, + ExtraGradientIter); they sum to
//    FUSED_POC_EXEC, the measured time, and PRED_EXEC_SOURCE says so
//    ("estimated-apportioned"; "measured" with --per-launch, which times each
//    launch as the reference does);
//  * extra keys after the reference's: FUSED_POC_EXEC, PRED_EXEC_SOURCE,
//    READ_CSV_TIME (ingest), LOG_WRITE_TIME (host time formatting + writing
//    the logs, overlapped with the GPU), LOG_BYTES.
//
// The units: cli_options (command line -> Settings), cli_plan (layout, POC
// dealing, batches, apportioning; both host-only), cli_worker (one device's
// work), and this file, the sequence that joins them.
#include <hip/hip_runtime.h>
#include <sys/time.h>
#include <time.h>

#include <cstdio>
#include <cstring>
#include <thread>

#include "cli_worker.h"

using namespace vame_cli;

namespace {

void print_timestamp(const char* msg) {
  struct timeval tv;
  gettimeofday(&tv, nullptr);
  struct tm* t = localtime(&tv.tv_sec);
  printf("%s @ %02d:%02d:%02d.%03d\n", msg, t->tm_hour, t->tm_min, t->tm_sec, (int)(tv.tv_usec / 1000));
}

// The OpenCL listing of main.cpp:133-247, as HIP, and the check of the chosen
// devices.  False (after the reference's message) if one does not exist.
bool list_devices(const std::vector<int>& devices) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
  for (int d = 0; d < ndev; d++) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, d) != hipSuccess) continue;
    printf("GPU %d\n\t%s (%s)\n", d, p.name, p.gcnArchName);
  }
  for (int d : devices)
    if (d < 0 || d >= ndev) {
      printf("Incorrect GPU index. Only %d GPUs are detected\n", ndev);
      return false;
    }
  for (int d : devices) {
    hipDeviceProp_t p;
    (void)hipGetDeviceProperties(&p, d);
    printf("COMPUTING ON GPU %d\n", d);
    printf("-- Max compute units %d\n", p.multiProcessorCount);
  }
  return true;
}

// main_aux_functions.h:1499-1545 testReferences (prints POC 1 .. N-1)
void test_references(int n_frames, int qp) {
  printf("-=-=-= Artificial references used for debugging =-=-=-=-\n");
  printf("Input QP = %d\n", qp);
  for (int f = 1; f < n_frames; f++) {
    int refs[4];
    const int n = vame_ref_list(f, refs);
    printf("POC %3d   QP %d motionLambda %f : [L0 %d", f, vame_poc_qp(qp, f), (double)vame_lambda(qp, f), refs[0]);
    for (int r = 1; r < n; r++) printf(" %d", refs[r]);
    printf("]\n");
  }
}

// The sample files into orig / recon (main.cpp:308-330); the seconds it took
// in *read_s.  False after its message.
bool ingest(const Settings& s, std::vector<uint16_t>& orig, std::vector<uint16_t>& recon, double* t_read0,
            double* read_s) {
  const size_t fsz = (size_t)s.W * s.H;
  orig.resize(fsz * s.frames);
  recon.resize(fsz * s.frames);
  FILE* a = fopen(s.orig_path.c_str(), "r");
  FILE* b = fopen(s.recon_path.c_str(), "r");
  if (!a || !b) {
    perror("error while opening samples files");
    return false;
  }
  fclose(a);
  fclose(b);
  print_timestamp("START READ .csv");
  *t_read0 = now_s();
  if (vame_read_frames(s.recon_path.c_str(), s.W, s.H, s.frames, recon.data(), s.threads) ||
      vame_read_frames(s.orig_path.c_str(), s.W, s.H, s.frames, orig.data(), s.threads)) {
    printf("  [!] ERROR: could not read %d frames of %dx%d from the sample files\n", s.frames, s.W, s.H);
    return false;
  }
  *read_s = now_s() - *t_read0;
  print_timestamp("FINISHED READ .csv");
  return true;
}

// Every worker's pinned slabs, each in its owner's pool.  False after its message.
bool allocate_slabs(const Settings& s, const Layout& L, std::vector<Slab>& slabs, Shared& S) {
  const int per_worker = slabs_per_worker(s.per_launch);
  slabs = std::vector<Slab>((size_t)per_worker * s.devices.size());
  S.pools.resize(s.devices.size());
  for (size_t i = 0; i < slabs.size(); i++) {
    Slab& slab = slabs[i];
    if (hipHostMalloc(slab.block.put(), L.bytes, hipHostMallocDefault) != hipSuccess) {
      printf("  [!] ERROR: pinned host allocation of %zu bytes failed\n", L.bytes);
      return false;
    }
    slab.owner = (int)(i / per_worker);
    S.pools[slab.owner].push_back(&slab);
  }
  return true;
}

struct Totals {  // what the writer loop sums over the POCs
  float pred_ns[4] = {0, 0, 0, 0}, fused_ns = 0;
  long long log_bytes = 0;
  double log_s = 0;
};

// One POC's report lines and log rows, every (refIdx, PRED) in the
// reference's order.  False after its message.
bool write_poc(const Settings& s, const Layout& L, vame_log_writer* logw, const Slab& slab, Totals& T) {
  const int p = slab.poc, predMask = vame_pred_mask(s.mode_mask);
  const float lambda = vame_lambda(s.qp, p);
  const int64_t* costs[16] = {};
  const vame_cpmvs* cps[16] = {};
  for (int r = 0; r < slab.nrefs; r++) {
    printf("POC   %d  RefIdx  %d  -> lambda %f\n", p, r, (double)lambda);
    for (int m = 0; m < 4; m++) {
      if (!((predMask >> m) & 1)) continue;
      printf("Reporting results POC=%d refIdx=%d PredType=%d\n", p, r, m);
      costs[r * 4 + m] = (const int64_t*)(slab.host() + L.off_cost[r][m]);
      cps[r * 4 + m] = (const vame_cpmvs*)(slab.host() + L.off_cp[r][m]);
      if (s.prefix.empty() || p != 1 || r != 0) continue;
      printf("Writing headers\n");
      if (vame_log_write_headers(s.prefix.c_str(), m)) {
        printf("  [!] ERROR: cannot create the log files %s_*\n", s.prefix.c_str());
        return false;
      }
    }
  }
  if (!logw) return true;
  const double tl = now_s();
  const long long nb = vame_log_writer_poc(logw, p, slab.nrefs, predMask, costs, cps);
  T.log_s += now_s() - tl;
  if (nb < 0) {
    printf("  [!] ERROR: writing the log files %s_* failed\n", s.prefix.c_str());
    return false;
  }
  T.log_bytes += nb;
  return true;
}

// The writer: POCs in order (main.cpp:954-958 -> main_aux_functions.h:387-525),
// a whole POC per vame_log_writer_poc call (persistent pool, files kept open),
// each slab back to its worker's pool.  False if a worker or the writer
// failed; the workers have then been told to stop.
bool write_pocs(const Settings& s, const Layout& L, vame_log_writer* logw, Shared& S, Totals& T) {
  bool ok = true;
  for (int p = 1; p <= s.frames && ok; p++) {
    Slab* slab = nullptr;
    {
      std::unique_lock<std::mutex> g(S.mu);
      S.cv.wait(g, [&] { return S.failed || S.done.count(p); });
      if (S.failed) {
        ok = false;
        break;
      }
      slab = S.done[p];
      S.done.erase(p);
    }
    ok = write_poc(s, L, logw, *slab, T);
    for (int m = 0; m < 4; m++) T.pred_ns[m] += slab->pred_ns[m];
    T.fused_ns += slab->fused_ns;
    memset(slab->pred_ns, 0, sizeof slab->pred_ns);
    slab->fused_ns = 0;
    std::lock_guard<std::mutex> g(S.mu);
    S.pools[slab->owner].push_back(slab);
    S.cv.notify_all();
  }
  if (!ok) {
    std::lock_guard<std::mutex> g(S.mu);
    S.failed = true;
    S.cv.notify_all();
  }
  return ok;
}

// main_aux_functions.h:1416-1446 reportTimingResults (ns; float like the reference)
void report_timing(const Settings& s, Totals& T, double overall, double read_s) {
  printf("=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=\n");
  printf("TIMING RESULTS (nanoseconds)\n");
  float* pred_ns = T.pred_ns;
  // fused launches: apportion by each PRED's algorithmic work
  if (!s.per_launch) apportion(T.fused_ns, s.W, s.H, vame_pred_mask(s.mode_mask), s.extra, pred_ns);
  printf("FULL_2CP_EXEC,%f\n", (double)pred_ns[0]);
  printf("FULL_3CP_EXEC,%f\n", (double)pred_ns[1]);
  printf("HALF_2CP_EXEC,%f\n", (double)pred_ns[2]);
  printf("HALF_3CP_EXEC,%f\n", (double)pred_ns[3]);
  const double total_ns =
      s.per_launch ? (double)(pred_ns[0] + pred_ns[1] + pred_ns[2] + pred_ns[3]) : (double)T.fused_ns;
  printf("TOTAL_EXEC_TIME(%dx),%f\n", s.frames, total_ns);
  printf("OVERALL(%dx),%f\n", s.frames, (double)(float)overall);
  if (!s.per_launch) printf("FUSED_POC_EXEC,%f\n", (double)T.fused_ns);
  // how the four per-PRED keys above were obtained: measured per launch
  // (--per-launch, the reference's events), or -- one fused launch computes
  // all four PREDs -- the measured fused time apportioned by algorithmic work
  printf("PRED_EXEC_SOURCE,%s\n", s.per_launch ? "measured" : "estimated-apportioned");
  printf("READ_CSV_TIME,%f\n", read_s * 1e9);
  printf("LOG_WRITE_TIME,%f\n", T.log_s * 1e9);
  printf("LOG_BYTES,%lld\n", T.log_bytes);
  printf("=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=-=\n\n");
}

}  // namespace

int main(int argc, char** argv) {
  Settings s;
  int rc = read_settings(argc, argv, s);
  if (rc >= 0) return rc;
  print_timestamp("START HOST");
  if (!list_devices(s.devices)) return 0;
  if ((rc = check_settings(s)) >= 0) return rc;
  test_references(s.frames, s.qp);

  std::vector<uint16_t> orig, recon;
  double t_read0 = 0, read_s = 0;
  if (!ingest(s, orig, recon, &t_read0, &read_s)) return 1;
  printf("Removing older outputs with identical names...\n");  // main.cpp:469 -> :1548
  vame_log_remove_old(s.prefix.c_str());

  // ---- shard POCs 1..N over the devices.  The slabs are declared before the
  // workers and outlive them on every return below: no worker is running
  // when they are freed.
  print_timestamp("START ALLOCATE MEMORY");
  const Layout L(vame_num_ctus(s.W, s.H));
  Shared S;
  std::vector<Slab> slabs;
  if (!allocate_slabs(s, L, slabs, S)) return 1;
  const std::vector<std::vector<int>> pocs = deal_pocs(s.frames, (int)s.devices.size());
  print_timestamp("FINISH ALLOCATE MEMORY");

  // the log writer (main.cpp:954-958 -> main_aux_functions.h:387-525) exists
  // before any worker starts, so a failure here returns with no thread running
  vame_log_writer* logw =
      s.prefix.empty() ? nullptr : vame_log_writer_create(s.prefix.c_str(), s.W, s.H, s.threads);
  if (!s.prefix.empty() && !logw) {
    printf("  [!] ERROR: cannot create the log writer for %s_*\n", s.prefix.c_str());
    return 1;
  }

  print_timestamp("START GPU KERNEL");
  const double t0 = now_s();
  std::vector<std::thread> workers;
  for (int g = 0; g < (int)s.devices.size(); g++)
    if (!pocs[g].empty())
      workers.emplace_back(gpu_worker, Job{g, s.devices[g], pocs[g], &s, orig.data(), recon.data(), &L, &S});
  Totals T;
  const bool ok = write_pocs(s, L, logw, S, T);
  for (auto& t : workers) t.join();
  if (logw) vame_log_writer_destroy(logw);
  fflush(stdout);
  if (!S.error.empty() || !ok) {
    printf("  [!] ERROR: %s\n", S.error.empty() ? "log writer failed" : S.error.c_str());
    return 1;
  }
  print_timestamp("FINISH GPU KERNEL");
  const double overall = now_s() - t0;
  if (trace_enabled())
    fprintf(stderr, "[trace] workers started %.1f ms after reading; overall %.1f ms, log writing %.1f ms\n",
            (t0 - t_read0 - read_s) * 1e3, overall * 1e3, T.log_s * 1e3);
  report_timing(s, T, overall, read_s);
  slabs.clear();
  print_timestamp("FINISH HOST");
  return 0;
}
