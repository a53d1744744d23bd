// cli_options.cpp -- see cli_options.h.  Every message and the help layout
// are the reference's (or, for the extensions, what the CLI has always
// printed): tests and profiles/ records match them character for character.
#include "cli_options.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>

#include "../../include/vame.h"

namespace vame_cli {

Cli::Cli()
    : opts{{
          {"DeviceIndex", 0, true, "0", "Index of the GPU device according ot clinfo command"},
          {"QP", 'q', false, "", "Quantization parameter"},
          {"FramesToBeEncoded", 'f', false, "", "Number of frames to be processed"},
          {"ExtraGradientIter", 0, true, "0", "Number of extra iterations during Gradient-based Affine ME"},
          {"Resolution", 's', false, "", "Resolution of the video, in the format 1920x1080"},
          {"OriginalFrames", 'o', false, "", "Input file for original frames samples"},
          {"ReferenceFrames", 'r', false, "", "Input file for reference frames samples"},
          {"CpmvLogFile", 'l', true, "", "Output files preffix with produced CPMVs"},
          {"gpus", 0, true, "1", "number of GPUs (POCs frame-sharded over DeviceIndex..+gpus-1)"},
          {"modes", 0, true, "all", "all = 2- and 3-CP affine, 2cp = 2-CP only"},
          {"align", 0, true, "both", "both = aligned (FULL) and half-aligned (HALF) CUs, full / half = one of them"},
          {"threads", 0, true, "0", "host threads for CSV parsing and log formatting (0 = all)"},
          {"devices", 0, true, "", "explicit device list, e.g. 0,1,2 (overrides DeviceIndex/gpus; "
                                   "a device may repeat: several contexts on one GPU)"},
      }} {}

int Cli::find(const std::string& n) const {
  for (size_t i = 0; i < opts.size(); i++)
    if (n == opts[i].name) return (int)i;
  // boost's allow_guessing: a unique prefix of a long option name
  int hit = -1;
  for (size_t i = 0; i < opts.size(); i++)
    if (strncmp(opts[i].name, n.c_str(), n.size()) == 0) {
      if (hit >= 0) return -2;
      hit = (int)i;
    }
  return hit;
}

int Cli::find_short(char c) const {
  for (size_t i = 0; i < opts.size(); i++)
    if (opts[i].shortc == c) return (int)i;
  return -1;
}

int Cli::num(OptId id) const { return atoi(str(id).c_str()); }

bool Cli::flag(const char* n) const { return std::find(flags_set.begin(), flags_set.end(), n) != flags_set.end(); }

void print_help(const Cli& c) {
  printf("Allowed options:\n");
  printf("  -h [ --help ]                         produce help message\n");
  for (auto& o : c.opts) {
    char lhs[96];
    if (o.shortc)
      snprintf(lhs, sizeof lhs, "  -%c [ --%s ] arg%s", o.shortc, o.name,
               o.has_default ? (" (=" + o.def + ")").c_str() : "");
    else
      snprintf(lhs, sizeof lhs, "  --%s arg%s", o.name, o.has_default ? (" (=" + o.def + ")").c_str() : "");
    printf("%-40s%s\n", lhs, o.help);
  }
  printf("%-40s%s\n", "  --per-launch", "one launch per (refIdx, PRED) like the reference (per-PRED kernel times)");
  printf("%-40s%s\n", "  --prof", "PROF on (the reference's enablePROF, hard-coded 0 there)");
}

int parse(Cli& c, int argc, const char* const* argv) {
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    int idx = -1;
    std::string val;
    bool have_val = false;
    if (a.size() > 2 && a[0] == '-' && a[1] == '-') {
      std::string n = a.substr(2);
      size_t eq = n.find('=');
      if (eq != std::string::npos) {
        val = n.substr(eq + 1);
        n = n.substr(0, eq);
        have_val = true;
      }
      if (n == "help") return 1;
      if (n == "per-launch" || n == "prof") {
        c.flags_set.push_back(n);
        continue;
      }
      idx = c.find(n);
      if (idx == -2) {
        fprintf(stderr, "option '--%s' is ambiguous\n", n.c_str());
        return 2;
      }
    } else if (a.size() >= 2 && a[0] == '-') {
      if (a[1] == 'h' && a.size() == 2) return 1;
      idx = c.find_short(a[1]);
      if (a.size() > 2) {
        val = a.substr(2);
        have_val = true;
      }
    } else {
      fprintf(stderr, "unexpected positional argument '%s'\n", a.c_str());
      return 2;
    }
    if (idx < 0) {
      fprintf(stderr, "unrecognised option '%s'\n", a.c_str());
      return 2;
    }
    if (!have_val) {
      if (i + 1 >= argc) {
        fprintf(stderr, "the required argument for option '--%s' is missing\n", c.opts[idx].name);
        return 2;
      }
      val = argv[++i];
    }
    c.opts[idx].set = true;
    c.opts[idx].val = val;
  }
  return 0;
}

int check_report(const Cli& c) {
  int errors = 0;
  printf("-=-= INPUT PARAMETERS =-=-\n");
  if (c.defaulted(kDeviceIndex))
    printf("  Device index not set. Using standard value of %d.\n", c.num(kDeviceIndex));
  else
    printf("  Device Index=%d\n", c.num(kDeviceIndex));
  if (c.defaulted(kLogFile))
    printf("  CPMVs log file not set. The output will not be written to any file.\n");
  else
    printf("  CpmvLogFile=%s\n", c.str(kLogFile).c_str());
  if (c.has(kQP))
    printf("  QP=%d\n", c.num(kQP));
  else {
    printf("  [!] ERROR: QP not set.\n");
    errors++;
  }
  if (c.has(kFrames))
    printf("  FramesToBeEncoded=%d\n", c.num(kFrames));
  else {
    printf("  [!] ERROR: FramesToBeEncoded not set.\n");
    errors++;
  }
  if (c.defaulted(kExtraIter))
    printf("  ExtraGradientIter not specified. Using zero extra gradients (i.e., 5 iterations for 2 "
           "CPs and 4 iterations for 3 CPs).\n");
  else {
    const int e = c.num(kExtraIter);
    printf("  ExtraGradientIter=%d. Using a total of %d iterations for 2 CPs and %d iterations for "
           "3 CPs.\n",
           e, 5 + e, 4 + e);
  }
  if (c.has(kResolution))
    printf("  Resolution=%s\n", c.str(kResolution).c_str());
  else {
    printf("  [!] ERROR: Resolution not set.\n");
    errors++;
  }
  if (c.has(kOrigFrames))
    printf("  InputOriginalFrame=%s\n", c.str(kOrigFrames).c_str());
  else {
    printf("  [!] ERROR: Input original frames not set.\n");
    errors++;
  }
  if (c.has(kRefFrames))
    printf("  InputReferenceFrame=%s\n", c.str(kRefFrames).c_str());
  else {
    printf("  [!] ERROR: Input reference frames not set.\n");
    errors++;
  }
  return errors;
}

namespace {

// "<W>x<H>" (main.cpp:285-294); false for any other number of x-separated parts
bool split_resolution(const std::string& res, int& W, int& H) {
  std::vector<std::string> tok;
  std::stringstream ss(res);
  for (std::string t; std::getline(ss, t, 'x');) tok.push_back(t);
  if (tok.size() != 2) return false;
  W = atoi(tok[0].c_str());
  H = atoi(tok[1].c_str());
  return true;
}

}  // namespace

int read_settings(int argc, const char* const* argv, Settings& s) {
  Cli c;
  const int pr = parse(c, argc, argv);
  if (pr == 1) print_help(c);
  if (pr != 0) return 1;
  if (check_report(c) > 0) {
    printf("Exiting after finding errors in input parameters\n");
    return 1;
  }
  const std::string& modes = c.str(kModes);
  if (modes != "all" && modes != "2cp") {
    printf("  [!] ERROR: --modes must be all or 2cp\n");
    return 1;
  }
  const std::string& align = c.str(kAlign);
  if (align != "both" && align != "full" && align != "half") {
    printf("  [!] ERROR: --align must be both, full or half\n");
    return 1;
  }
  s.mode_mask = (modes == "all" ? (VAME_MODE_2CP | VAME_MODE_3CP) : VAME_MODE_2CP) |
                (align == "full" ? VAME_MODE_FULL : align == "half" ? VAME_MODE_HALF : 0);
  s.per_launch = c.flag("per-launch");
  s.prof = c.flag("prof");
  s.threads = c.num(kThreads);
  s.devices.clear();
  if (!c.str(kDevices).empty()) {
    std::stringstream ss(c.str(kDevices));
    for (std::string t; std::getline(ss, t, ',');) s.devices.push_back(atoi(t.c_str()));
  } else {
    for (int g = 0; g < std::max(1, c.num(kGpus)); g++) s.devices.push_back(c.num(kDeviceIndex) + g);
  }
  s.frames = c.num(kFrames);
  s.qp = c.num(kQP);
  s.extra = c.num(kExtraIter);
  s.resolution = c.str(kResolution);
  s.W = s.H = 0;
  (void)split_resolution(s.resolution, s.W, s.H);
  s.orig_path = c.str(kOrigFrames);
  s.recon_path = c.str(kRefFrames);
  s.prefix = c.str(kLogFile);
  return -1;
}

int check_settings(const Settings& s) {
  int W, H;
  if (!split_resolution(s.resolution, W, H)) {
    printf("  [!] ERROR: Input resolution \"%s\" not set properly\n", s.resolution.c_str());
    return 0;
  }
  if (vame_num_ctus(W, H) == 0) {
    printf("[!] ERROR: Unsupported resolution %dx%d\n", W, H);
    printf("Supported resolutions are:\n");
    const int rs[5][2] = {{3840, 2160}, {1920, 1080}, {1280, 720}, {832, 480}, {416, 240}};
    for (auto& r : rs) printf("  %dx%d\n", r[0], r[1]);
    return 0;
  }
  if (s.frames <= 0) {
    printf("  [!] ERROR: FramesToBeEncoded must be positive\n");
    return 1;
  }
  if (vame_lambda(s.qp, 1) < 0 || vame_lambda(s.qp, 8) < 0) {
    printf("  [!] ERROR: QP %d outside the lambda table\n", s.qp);
    return 1;
  }
  return -1;
}

}  // namespace vame_cli
