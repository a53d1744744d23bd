// cli_options.h -- the `vame` CLI's command line: the reference's boost-style
// options (main.cpp:53-131) plus the extensions listed in vame_main.cpp's
// header, its parameter report, and the Settings everything else reads.
// Host-only (no HIP): tests/native/cli_check.cpp runs it under ASan + UBSan.
#pragma once
#include <array>
#include <string>
#include <vector>

namespace vame_cli {

// The options that take a value, in the order of the table (Cli::Cli) and of
// the help text.
enum OptId {
  kDeviceIndex, kQP, kFrames, kExtraIter, kResolution, kOrigFrames, kRefFrames, kLogFile,
  kGpus, kModes, kAlign, kThreads, kDevices, kNumOpts
};

struct Opt {
  const char* name;
  char shortc;
  bool has_default;
  std::string def;
  const char* help;
  bool set = false;
  std::string val;
};

struct Cli {
  std::array<Opt, kNumOpts> opts;      // opts[id] is option id
  std::vector<std::string> flags_set;  // value-less extension flags
  Cli();
  // parse() only: an index, -1 (unknown) or -2 (ambiguous prefix)
  int find(const std::string& n) const;
  int find_short(char c) const;
  bool has(OptId id) const { return opts.at(id).set; }
  bool defaulted(OptId id) const { return !has(id); }
  const std::string& str(OptId id) const { return has(id) ? opts.at(id).val : opts.at(id).def; }
  int num(OptId id) const;
  bool flag(const char* n) const;
};

void print_help(const Cli& c);
// Returns 0 ok, 1 help, 2 error.
int parse(Cli& c, int argc, const char* const* argv);
// main_aux_functions.h:77-145 checkReportParameters; returns the error count
int check_report(const Cli& c);

// What the run reads from the command line.
struct Settings {
  int frames = 0, qp = 0, extra = 0;
  std::string resolution;  // as given
  int W = 0, H = 0;        // 0 x 0 if it is not of the form <W>x<H>
  std::string orig_path, recon_path, prefix;
  int mode_mask = 0;
  bool per_launch = false, prof = false;
  int threads = 0;
  std::vector<int> devices;  // one worker each: --devices, or DeviceIndex .. +gpus-1
};

// Parses the command line, prints the reference's report (or the help, or the
// parser's error) and fills s.  Returns -1 to go on, else the exit code.
int read_settings(int argc, const char* const* argv, Settings& s);
// The checks the reference makes after its device listing (main.cpp:285-306)
// and ours of the frame count and the QP, with their messages.  Returns -1 to
// go on, else the exit code.
int check_settings(const Settings& s);

}  // namespace vame_cli
