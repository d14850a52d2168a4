// hevcdl_app.cpp -- command-line front end with the reference application's surface.
//
// Accepts what the reference is started with,  TAppEncoder -c encoder_intra_main.cfg -c bitstream.cfg [-q QP ...]
//   option syntax                HM_dl/source/Lib/TAppCommon/program_options_lite.cpp (cfg "Key : value  # comment",
//                                "--Key=value" / "--Key value", short options)
//   option names / short forms   HM_dl/source/App/TAppEncoder/TAppEncCfg.cpp:730-1290
//   planar YUV reader            HM_dl/source/Lib/TLibVideoIO/TVideoIOYuv.cpp:249,675 (8-bit 4:2:0 file, FrameSkip)
//   padding / window / depths    TAppEncCfg.cpp:1569-1632 (ConformanceWindowMode 0 / 1 / 2), TVideoIOYuv.cpp:70-95, 363-381, 755-830: the file holds source-format frames, the
//                                library pads and converts them on the device (hevcdl_set_source_format), the reconstruction file holds the window at OutputBitDepth
//   file layout                  TVideoIOYuv.cpp:249-384 (InputChromaFormat 400 / 422 / 444 into a 4:2:0 coded picture), :981-1041 (InputColourSpaceConvert YCbCrtoYCrCb),
//                                TAppEncCfg.cpp:1618-1631 (ConformanceWindowMode 3 with ConfWin*), TAppEncTop.cpp:669 + TAppEncCfg.cpp:1286 (TemporalSubsampleRatio)
//   picture log line / summary   TEncGOP.cpp:2500-2541, TEncAnalyze.h:163-370
// and drives the GPU path through the C ABI of include/hevcdl.h only.  Keys that would change the path are checked
// against what the path implements (rejected, not ignored).  Labels come from the on-device CNN, or -- the reference's own
// file IPC format -- from --LabelDir <dir>/<frame>/ctu<addr>.txt (16 integers, TEncCu.cpp:255-262).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>
#include <functional>
#include <dlfcn.h>
#include <sys/types.h>
#include <sstream>
#include <string>
#include <atomic>
#include <thread>
#include <vector>
#include "hevcdl.h"
#include "slice_grid.h"      // hevcdl_segment_keys: the segment keys are refused here with the library's own sentences
#include "qp_rd.h"           // hevcdl_qp_rd_keys: likewise DeltaQpRD
#include "frame_qp.h"        // the rule of a QP per picture (dQPFile, QPIncrementFrame, IntraQPOffset, LambdaModifierI / 0) and its refusals

namespace {

enum Kind { USED, PATH, STAGE, NOEFFECT };
struct Key { const char *name; const char *shortopt; Kind kind; const char *required; };   // required: value the path implements (PATH)

const Key KEYS[] = {
  // used by this front end
  { "InputFile", "i", USED, 0 }, { "BitstreamFile", "b", USED, 0 }, { "ReconFile", "o", USED, 0 }, { "SourceWidth", "wdt", USED, 0 },
  { "SourceHeight", "hgt", USED, 0 }, { "FrameRate", "fr", USED, 0 }, { "FrameSkip", "fs", USED, 0 }, { "FramesToBeEncoded", "f", USED, 0 },
  { "QP", "q", USED, 0 },
  // a QP per picture (TAppEncCfg.cpp:866, 871, 899, 853, 860; csrc/frame_qp.h): the offsets are computed once for the sequence, every batch sets its slice (hevcdl_set_frame_qps)
  { "dQPFile", "m", USED, 0 }, { "QPIncrementFrame", "qpif", USED, 0 }, { "IntraQPOffset", 0, USED, 0 }, { "LambdaModifierI", "LMI", USED, 0 }, { "LambdaModifier0", "LM0", USED, 0 },
  // extensions of this front end
  { "LabelDir", 0, USED, 0 }, { "BatchFrames", 0, USED, 0 }, { "ChunkFrames", 0, USED, 0 }, { "Device", 0, USED, 0 }, { "Devices", 0, USED, 0 }, { "NumDevices", 0, USED, 0 }, { "Weights", 0, USED, 0 }, { "RecordFile", 0, USED, 0 }, { "DeviceEntropy", 0, USED, 0 }, { "DeviceReport", 0, USED, 0 },
  { "CnnInput", 0, USED, 0 }, { "BnMode", 0, USED, 0 }, { "PrintConfig", 0, USED, 0 }, { "LoopFilterDisable", 0, USED, 0 },
  // keys that define the path: only the implemented value is accepted
  { "ConformanceWindowMode", 0, USED, 0 }, { "HorizontalPadding", "pdx", USED, 0 }, { "VerticalPadding", "pdy", USED, 0 }, { "OutputBitDepth", 0, USED, 0 }, { "OutputBitDepthC", 0, USED, 0 },
  { "ConfWinLeft", 0, USED, 0 }, { "ConfWinRight", 0, USED, 0 }, { "ConfWinTop", 0, USED, 0 }, { "ConfWinBottom", 0, USED, 0 },      // (ConformanceWindowMode 3 only)
  { "InputBitDepth", 0, USED, 0 }, { "InternalBitDepth", 0, USED, 0 }, { "InputChromaFormat", 0, USED, 0 }, { "ChromaFormatIDC", "cf", USED, 0 }, { "Profile", 0, USED, 0 },
  { "InputColourSpaceConvert", 0, USED, 0 }, { "OutputInternalColourSpace", 0, USED, 0 }, { "SNRInternalColourSpace", 0, USED, 0 }, { "TemporalSubsampleRatio", "ts", USED, 0 },
  { "MaxCUWidth", 0, PATH, "64" }, { "MaxCUHeight", 0, PATH, "64" }, { "MaxPartitionDepth", 0, PATH, "4" },
  { "QuadtreeTULog2MaxSize", 0, PATH, "5" }, { "QuadtreeTULog2MinSize", 0, PATH, "2" }, { "QuadtreeTUMaxDepthIntra", 0, PATH, "3" },
  { "IntraPeriod", 0, PATH, "1" }, { "GOPSize", 0, PATH, "1" }, { "MaxDeltaQP", 0, PATH, "0" }, { "DeltaQpRD", "dqr", USED, 0 },      // (DeltaQpRD: 0 .. 6, the slice QP of every picture picked among 2N+1 candidate encodes)
  { "RDOQ", 0, USED, 0 }, { "RDOQTS", 0, USED, 0 }, { "TransformSkip", 0, USED, 0 }, { "TransformSkipFast", 0, USED, 0 },
  { "SignHideFlag", "SBH", USED, 0 }, { "StrongIntraSmoothing", 0, USED, 0 }, { "FastUDIUseMPMEnabled", 0, USED, 0 },      // tool switches (hevcdl_config.tools): 0 or 1
  { "SliceMode", 0, USED, 0 }, { "SliceArgument", 0, USED, 0 }, { "SliceSegmentMode", 0, USED, 0 }, { "SliceSegmentArgument", 0, USED, 0 }, { "PCMEnabledFlag", 0, PATH, "0" }, { "NumTileColumnsMinus1", 0, USED, 0 },
  { "NumTileRowsMinus1", 0, USED, 0 }, { "WaveFrontSynchro", 0, USED, 0 }, { "ScalingList", 0, PATH, "0" },
  { "TransquantBypassEnable", 0, PATH, "0" }, { "CUTransquantBypassFlagForce", 0, PATH, "0" },
  // stream / in-loop filter keys
  { "Level", 0, USED, 0 }, { "DecodingRefreshType", 0, PATH, "1" }, { "ReWriteParamSetsFlag", 0, USED, 0 }, { "LoopFilterOffsetInPPS", 0, USED, 0 },
  { "LoopFilterBetaOffset_div2", 0, USED, 0 }, { "LoopFilterTcOffset_div2", 0, USED, 0 },
  { "DeblockingFilterMetric", 0, USED, 0 }, { "SAO", 0, USED, 0 }, { "SAOLcuBoundary", 0, PATH, "0" }, { "LFCrossSliceBoundaryFlag", 0, USED, 0 },      // (used with SliceMode 1 / 3; without slices the reference sets it to 1 whatever the cfg says: TAppEncTop.cpp:278-281)
  { "LFCrossTileBoundaryFlag", 0, USED, 0 }, { "SEIDecodedPictureHash", 0, USED, 0 },
  // quality report (TAppEncCfg.cpp:759-762): MS-SSIM per picture and in the summary, MSE per picture, MSE in the summary; default 0
  { "PrintMSSSIM", 0, USED, 0 }, { "PrintFrameMSE", 0, USED, 0 }, { "PrintSequenceMSE", 0, USED, 0 },
  // no effect on an all-intra slice with the settings above
  { "QuadtreeTUMaxDepthInter", 0, NOEFFECT, 0 }, { "FastSearch", 0, NOEFFECT, 0 }, { "SearchRange", 0, NOEFFECT, 0 }, { "HadamardME", 0, NOEFFECT, 0 },
  { "FEN", 0, NOEFFECT, 0 }, { "FDM", 0, NOEFFECT, 0 }, { "AMP", 0, NOEFFECT, 0 }, { "MaxCuDQPDepth", 0, NOEFFECT, 0 },
  { "PCMLog2MaxSize", 0, NOEFFECT, 0 }, { "PCMLog2MinSize", 0, NOEFFECT, 0 }, { "PCMInputBitDepthFlag", 0, NOEFFECT, 0 },
  { "PCMFilterDisableFlag", 0, NOEFFECT, 0 }, { "TileUniformSpacing", 0, USED, 0 }, { "TileColumnWidthArray", 0, USED, 0 },
  { "TileRowHeightArray", 0, USED, 0 }, { "ScalingListFile", 0, NOEFFECT, 0 },
  // lambda keys that an all-intra GOP of 1 never reads (TEncSlice.cpp:459-474: temporal layers above 0 do not exist, an I slice of an I GOP entry takes 0.57 whatever
  // IQPFactor says, and LambdaFromQpEnable picks the same 0.57 with no B pictures)
  { "LambdaModifier1", "LM1", NOEFFECT, 0 }, { "LambdaModifier2", "LM2", NOEFFECT, 0 }, { "LambdaModifier3", "LM3", NOEFFECT, 0 }, { "LambdaModifier4", "LM4", NOEFFECT, 0 },
  { "LambdaModifier5", "LM5", NOEFFECT, 0 }, { "LambdaModifier6", "LM6", NOEFFECT, 0 }, { "IQPFactor", "IQF", NOEFFECT, 0 }, { "LambdaFromQpEnable", 0, NOEFFECT, 0 },
};

const Key *find_key(const std::string &name, bool shortform)
{
  for (const Key &k : KEYS) if (shortform ? (k.shortopt && name == k.shortopt) : name == k.name) return &k;
  return nullptr;
}

std::string trim(const std::string &s)
{
  size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
  return a == std::string::npos ? "" : s.substr(a, b - a + 1);
}

struct Options {
  std::map<std::string, std::string> v;
  std::vector<std::string> errors;
  void set(const std::string &name, const std::string &val, bool shortform, const std::string &where)
  {
    const Key *k = find_key(name, shortform);
    if (!k) { errors.push_back(where + ": unknown option '" + name + "'"); return; }
    v[k->name] = val;
  }
  bool parse_cfg(const std::string &path)
  { // program_options_lite::scanFile: "name : value", '#' starts a comment, blank lines ignored
    std::ifstream f(path);
    if (!f) { errors.push_back("cannot open configuration file '" + path + "'"); return false; }
    std::string line; int ln = 0;
    while (std::getline(f, line)) {
      ln++;
      const size_t h = line.find('#'); if (h != std::string::npos) line.erase(h);
      line = trim(line); if (line.empty()) continue;
      const size_t c = line.find(':');
      if (c == std::string::npos) { errors.push_back(path + ":" + std::to_string(ln) + ": expected 'name : value'"); continue; }
      set(trim(line.substr(0, c)), trim(line.substr(c + 1)), false, path + ":" + std::to_string(ln));
    }
    return true;
  }
  void parse_argv(int argc, char **argv)
  {
    for (int i = 1; i < argc; i++) {
      std::string a = argv[i];
      if (a == "-c") { if (i + 1 < argc) parse_cfg(argv[++i]); else errors.push_back("-c needs a file"); continue; }
      if (a.rfind("--", 0) == 0) {
        const size_t e = a.find('=');
        if (e != std::string::npos) set(a.substr(2, e - 2), a.substr(e + 1), false, "command line");
        else if (a.substr(2) == "PrintConfig") set("PrintConfig", "1", false, "command line");
        else if (i + 1 < argc) { set(a.substr(2), argv[i + 1], false, "command line"); i++; }
        else errors.push_back("option '" + a + "' needs a value");
      } else if (a.size() > 1 && a[0] == '-') {
        if (i + 1 < argc) { set(a.substr(1), argv[i + 1], true, "command line"); i++; }
        else errors.push_back("option '" + a + "' needs a value");
      } else errors.push_back("stray argument '" + a + "'");
    }
  }
  std::string get(const char *k, const char *dflt = "") const { auto it = v.find(k); return it == v.end() ? dflt : it->second; }
  long geti(const char *k, long dflt) const { auto it = v.find(k); return it == v.end() ? dflt : strtol(it->second.c_str(), nullptr, 10); }
};

std::string native_path(std::string p)
{ // the reference's cfg files carry Windows paths (".\rec\rec.yuv")
  std::replace(p.begin(), p.end(), '\\', '/');
  return p;
}

double psnr_of(unsigned long long sse, double n, double maxval = 255.0) { return sse == 0 ? 999.99 : 10.0 * log10(maxval * maxval * n / (double)sse); }   // TEncGOP.cpp:2391-2393, maxval = 255 << (bitDepth - 8)

std::string json_escape(const std::string &s) { std::string o; for (char c : s) { if (c == '"' || c == '\\') o += '\\'; o += c; } return o; }

// ---- RCCL from C++: the per-picture rows of every device in one all-gather -------------------------------------------------------------------
// librccl and the HIP runtime are opened at run time (a single-device run needs neither); the handful of entry points used are declared here with their ABI types
// (rccl.h: ncclResult_t / ncclDataType_t are ints, ncclComm_t and hipStream_t opaque pointers; ncclUint64 = 5).
struct RcclApi {
  void *h_rccl = nullptr, *h_hip = nullptr;
  int (*CommInitAll)(void **comms, int ndev, const int *devlist) = nullptr;
  int (*CommDestroy)(void *comm) = nullptr;
  int (*AllGather)(const void *send, void *recv, size_t count, int datatype, void *comm, void *stream) = nullptr;
  int (*GroupStart)() = nullptr; int (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
  int (*GetVersion)(int *) = nullptr; int (*CommCount)(void *comm, int *count) = nullptr;
  int (*hipSetDevice)(int) = nullptr; int (*hipMalloc)(void **, size_t) = nullptr; int (*hipFree)(void *) = nullptr;
  int (*hipMemcpy)(void *, const void *, size_t, int) = nullptr; int (*hipDeviceSynchronize)() = nullptr;
  bool load(std::string &err)
  {
    h_rccl = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL); if (!h_rccl) h_rccl = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    h_hip = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h_rccl || !h_hip) { err = std::string("cannot load ") + (h_rccl ? "libamdhip64.so" : "librccl.so") + ": " + dlerror(); return false; }
#define SYM(lib, field, name) do { *(void **)&field = dlsym(lib, name); if (!field) { err = std::string("missing symbol ") + name; return false; } } while (0)
    SYM(h_rccl, CommInitAll, "ncclCommInitAll"); SYM(h_rccl, CommDestroy, "ncclCommDestroy"); SYM(h_rccl, AllGather, "ncclAllGather");
    SYM(h_rccl, GroupStart, "ncclGroupStart"); SYM(h_rccl, GroupEnd, "ncclGroupEnd"); SYM(h_rccl, GetErrorString, "ncclGetErrorString");
    SYM(h_rccl, GetVersion, "ncclGetVersion"); SYM(h_rccl, CommCount, "ncclCommCount");
    SYM(h_hip, hipSetDevice, "hipSetDevice"); SYM(h_hip, hipMalloc, "hipMalloc"); SYM(h_hip, hipFree, "hipFree"); SYM(h_hip, hipMemcpy, "hipMemcpy");
    SYM(h_hip, hipDeviceSynchronize, "hipDeviceSynchronize");
#undef SYM
    return true;
  }
};

// rows_of(i): the rows (row_words 64-bit words each) of block i, coded on device dev_of(i).  -> table: every rank's contribution, padded with rows whose first word is ~0
// info: what ran, for the log -- the library's version, the size the communicator reports (ncclCommCount), the devices
bool gather_rows_rccl(size_t n_blocks, const std::function<int(size_t)> &dev_of, const std::function<const std::vector<unsigned long long> &(size_t)> &rows_of, int row_words,
                      std::vector<unsigned long long> &table, std::string &err, std::string *info = nullptr)
{
  RcclApi api;
  if (!api.load(err)) return false;
  std::vector<int> ranks;                                  // physical devices, in order of first appearance: one RCCL rank each
  for (size_t i = 0; i < n_blocks; i++) if (std::find(ranks.begin(), ranks.end(), dev_of(i)) == ranks.end()) ranks.push_back(dev_of(i));
  const int R = (int)ranks.size();
  std::vector<std::vector<unsigned long long>> contrib(R);
  for (size_t i = 0; i < n_blocks; i++) { auto &c = contrib[std::find(ranks.begin(), ranks.end(), dev_of(i)) - ranks.begin()]; const auto &r = rows_of(i); c.insert(c.end(), r.begin(), r.end()); }
  size_t words = (size_t)row_words;
  for (const auto &c : contrib) words = std::max(words, c.size());
  for (auto &c : contrib) c.resize(words, ~0ull);
  std::vector<void *> comms(R, nullptr), d_send(R, nullptr), d_recv(R, nullptr);
  auto cleanup = [&]() { for (int r = 0; r < R; r++) { api.hipSetDevice(ranks[r]); if (d_send[r]) api.hipFree(d_send[r]); if (d_recv[r]) api.hipFree(d_recv[r]); if (comms[r]) api.CommDestroy(comms[r]); } };
  auto fail = [&](const std::string &what, int code, bool nccl) { err = what + (nccl ? std::string(": ") + api.GetErrorString(code) : " failed (hip error " + std::to_string(code) + ")"); cleanup(); return false; };
  int e = api.CommInitAll(comms.data(), R, ranks.data());
  if (e) { std::fill(comms.begin(), comms.end(), nullptr); return fail("ncclCommInitAll", e, true); }
  for (int r = 0; r < R; r++) {
    if ((e = api.hipSetDevice(ranks[r]))) return fail("hipSetDevice", e, false);
    if ((e = api.hipMalloc(&d_send[r], words * 8)) || (e = api.hipMalloc(&d_recv[r], words * 8 * (size_t)R))) return fail("hipMalloc", e, false);
    if ((e = api.hipMemcpy(d_send[r], contrib[r].data(), words * 8, 1 /* hipMemcpyHostToDevice */))) return fail("hipMemcpy", e, false);
  }
  if ((e = api.GroupStart())) return fail("ncclGroupStart", e, true);
  for (int r = 0; r < R; r++) { api.hipSetDevice(ranks[r]); if ((e = api.AllGather(d_send[r], d_recv[r], words, 5 /* ncclUint64 */, comms[r], nullptr))) { api.GroupEnd(); return fail("ncclAllGather", e, true); } }
  if ((e = api.GroupEnd())) return fail("ncclGroupEnd", e, true);
  for (int r = 0; r < R; r++) { api.hipSetDevice(ranks[r]); if ((e = api.hipDeviceSynchronize())) return fail("hipDeviceSynchronize", e, false); }
  table.resize(words * (size_t)R);
  api.hipSetDevice(ranks[0]);
  if ((e = api.hipMemcpy(table.data(), d_recv[0], words * 8 * (size_t)R, 2 /* hipMemcpyDeviceToHost */))) return fail("hipMemcpy", e, false);
  if (info) {
    int ver = 0, cnt = 0; api.GetVersion(&ver); api.CommCount(comms[0], &cnt);
    char b[256]; int o = snprintf(b, sizeof b, "ncclAllGather over %d rank%s (ncclCommCount %d, RCCL/NCCL version code %d, one rank per physical device:", R, R == 1 ? "" : "s", cnt, ver);
    for (int r = 0; r < R && o < (int)sizeof b - 8; r++) o += snprintf(b + o, sizeof b - o, " %d", ranks[r]);
    snprintf(b + o, sizeof b - o, "), %zu words each", words);
    *info = b;
  }
  cleanup();
  return true;
}

} // namespace

int main(int argc, char **argv)
{
  const std::chrono::steady_clock::time_point t_main0 = std::chrono::steady_clock::now();
  Options opt;
  opt.parse_argv(argc, argv);
  // keys that define the path must carry the implemented value
  std::vector<std::string> stage_keys;
  for (const auto &kv : opt.v) {
    const Key *k = find_key(kv.first, false);
    if (k->kind == PATH && kv.second != k->required)
      opt.errors.push_back(std::string(k->name) + " = " + kv.second + " is not implemented by this path (only " + k->required + ")");
    if (k->kind == STAGE) stage_keys.push_back(k->name);
  }
  // SourceWidth / SourceHeight are the FILE's size; the context is created with the padded (coded) size of ConformanceWindowMode (TAppEncCfg.cpp:1569-1617): 0 none,
  // 1 up to the next multiple of the minimum CU (8), 2 by HorizontalPadding / VerticalPadding; 3: no padding, the window is the four ConfWin* offsets
  const int src_w = (int)opt.geti("SourceWidth", 0), src_h = (int)opt.geti("SourceHeight", 0), qp = (int)opt.geti("QP", 30);
  const int conf_mode = (int)opt.geti("ConformanceWindowMode", 0), pad_x = (int)opt.geti("HorizontalPadding", 0), pad_y = (int)opt.geti("VerticalPadding", 0);
  int width = src_w, height = src_h;
  const int win_l = conf_mode == 3 ? (int)opt.geti("ConfWinLeft", 0) : 0, win_r = conf_mode == 3 ? (int)opt.geti("ConfWinRight", 0) : 0;
  const int win_t = conf_mode == 3 ? (int)opt.geti("ConfWinTop", 0) : 0, win_b = conf_mode == 3 ? (int)opt.geti("ConfWinBottom", 0) : 0;
  if (conf_mode == 3) { // TAppEncCfg.cpp:1618-1631: nothing is padded, so the size must be the coded size already; the offsets are in luma samples and even (4:2:0, :2231-2234)
    if (src_w > 0 && src_h > 0 && ((src_w & 7) || (src_h & 7))) opt.errors.push_back("ConformanceWindowMode = 3 pads nothing: SourceWidth x SourceHeight must be multiples of the minimum CU (8)");
    if (win_l < 0 || win_r < 0 || win_t < 0 || win_b < 0 || ((win_l | win_r | win_t | win_b) & 1)) opt.errors.push_back("ConfWinLeft / ConfWinRight / ConfWinTop / ConfWinBottom: a conformance window offset must be an integer multiple of the specified chroma subsampling (2), and not negative");
    else if (src_w > 0 && src_h > 0 && (win_l + win_r >= src_w || win_t + win_b >= src_h)) opt.errors.push_back("ConfWinLeft / ConfWinRight / ConfWinTop / ConfWinBottom leave nothing of the picture");
  }
  else if (conf_mode < 0 || conf_mode > 3) opt.errors.push_back("ConformanceWindowMode = " + std::to_string(conf_mode) + " is not a value of the key (0, 1, 2 or 3)");
  else if (src_w > 0 && src_h > 0 && hevcdl_padded_size(src_w, src_h, conf_mode, pad_x, pad_y, &width, &height) != HEVCDL_OK)
    opt.errors.push_back("SourceWidth x SourceHeight with ConformanceWindowMode " + std::to_string(conf_mode) + ": the size must be even and the padded size a multiple of 8, the padding even and not negative");
  for (const char *key : { "ConfWinLeft", "ConfWinRight", "ConfWinTop", "ConfWinBottom" })
    if (conf_mode != 3 && opt.v.count(key)) opt.errors.push_back(std::string(key) + " belongs to ConformanceWindowMode 3");
  const long frame_skip = opt.geti("FrameSkip", 0); long n_frames = opt.geti("FramesToBeEncoded", 0);
  const double fps = atof(opt.get("FrameRate", "30").c_str());
  const std::string input = native_path(opt.get("InputFile")), recon_path = native_path(opt.get("ReconFile")), label_dir = native_path(opt.get("LabelDir"));
  const std::string cnn_input = opt.get("CnnInput", "rgb601");
  const std::string bitstream_path = native_path(opt.get("BitstreamFile"));
  const int level_idc = (int)(atof(opt.get("Level", "6.2").c_str()) * 30.0 + 0.5);      // general_level_idc
  const bool deblock = opt.geti("LoopFilterDisable", 0) == 0;
  const bool sao = opt.geti("SAO", 1) != 0;                                    // TAppEncCfg.cpp: SAO defaults to on
  const bool filtered = deblock || sao;      // an in-loop filter is on: the log's PSNR is the output picture's, not the reconstruction's before the filters (LoopFilterDisable 1 leaves SAO on)
  // sample bit depth (TAppEncCfg.cpp:770-780): 8 (Profile main) or 10 (Profile main10; the file then holds 16-bit little-endian samples).
  // InternalBitDepth 0 = the input's; OutputBitDepth 0 = the internal one (the reconstruction file's).  The file's samples are scaled to the internal depth on the device and
  // the output back as TVideoIOYuv.cpp:70-95 does: up by a shift, down by a rounding shift and a clip.
  const int in_bd = (int)opt.geti("InputBitDepth", 8), bit_depth = opt.geti("InternalBitDepth", 0) == 0 ? in_bd : (int)opt.geti("InternalBitDepth", 0);
  const int out_bd = opt.geti("OutputBitDepth", 0) == 0 ? bit_depth : (int)opt.geti("OutputBitDepth", 0);
  // (the reference's OutputBitDepthC defaults to the INTERNAL depth, not to OutputBitDepth: an output depth of its own has to be named for both channels, as chroma-specific
  // depths are not implemented)
  if ((opt.geti("OutputBitDepthC", 0) == 0 ? bit_depth : (int)opt.geti("OutputBitDepthC", 0)) != out_bd)
    opt.errors.push_back("OutputBitDepthC must equal OutputBitDepth on this path (it defaults to the internal depth, as in the reference; chroma-specific depths are not implemented)");
  if (in_bd < 8 || in_bd > 16) opt.errors.push_back("InputBitDepth = " + std::to_string(in_bd) + " is not implemented by this path (8 .. 16)");
  if (out_bd < 8 || out_bd > 16) opt.errors.push_back("OutputBitDepth = " + std::to_string(out_bd) + " is not implemented by this path (8 .. 16)");
  if (bit_depth != 8 && bit_depth != 10) opt.errors.push_back("InternalBitDepth = " + std::to_string(bit_depth) + " is not implemented by this path (only 8 and 10)");
  { const std::string prof = opt.get("Profile", bit_depth == 8 ? "main" : "main10");
    if (prof != (bit_depth == 8 ? "main" : "main10")) opt.errors.push_back("Profile = " + prof + " does not go with InternalBitDepth = " + std::to_string(bit_depth) + " on this path (main at 8 bits, main10 at 10 bits)"); }
  // The file's layout.  The coded picture is 4:2:0 (Profile main / main10), so ChromaFormatIDC must say 420 -- and must be named when the file is something else, because
  // the reference's default (0) means "as the input" and it then refuses the profile with the message below (TAppEncCfg.cpp:1381, 2033).
  const int in_cf = (int)opt.geti("InputChromaFormat", 420), cf_idc = (int)opt.geti("ChromaFormatIDC", 0);
  if (in_cf != 400 && in_cf != 420 && in_cf != 422 && in_cf != 444) opt.errors.push_back("InputChromaFormatIDC must be either 400, 420, 422 or 444");
  else if ((cf_idc == 0 ? in_cf : cf_idc) != 420) {
    if (cf_idc != 0 && cf_idc != 400 && cf_idc != 422 && cf_idc != 444) opt.errors.push_back("ChromaFormatIDC must be either 400, 420, 422 or 444");
    else opt.errors.push_back("ChromaFormatConstraint must be 420 for non main-RExt profiles.");
  }
  const std::string csc = opt.get("InputColourSpaceConvert", "");
  if (csc != "" && csc != "UNCHANGED" && csc != "YCbCrtoYCrCb") opt.errors.push_back("InputColourSpaceConvert = " + csc + " is not implemented by this path (only UNCHANGED and YCbCrtoYCrCb: the others need a 4:4:4 coded picture)");
  const int colour_space = csc == "YCbCrtoYCrCb" ? 1 : 0;
  if (colour_space && in_cf == 400) opt.errors.push_back("InputColourSpaceConvert = YCbCrtoYCrCb needs a file with chroma planes (InputChromaFormat 400 has none)");
  const int out_internal_cs = opt.geti("OutputInternalColourSpace", 0) != 0, snr_internal_cs = opt.geti("SNRInternalColourSpace", 0) != 0;
  // TemporalSubsampleRatio: the file reader skips ratio - 1 frames behind every picture it reads, and FramesToBeEncoded counts SOURCE frames (TAppEncTop.cpp:669, TAppEncCfg.cpp:1286);
  // the summary's bitrate is taken at FrameRate / ratio (TEncGOP.cpp:2043)
  const long ts_ratio = opt.geti("TemporalSubsampleRatio", 1);
  if (ts_ratio < 1) opt.errors.push_back("Temporal subsample rate must be no less than 1");
  // the source format goes to the library only when the file is not in the codec's own format already: every other run is the run it was
  const bool use_fmt = src_w != width || src_h != height || in_bd != bit_depth || out_bd != bit_depth || in_cf != 420 || colour_space || (win_l | win_r | win_t | win_b) != 0;
  const bool file_order = colour_space && !snr_internal_cs;      // the U and V columns are the file's second and third plane (the library's quality and report results come in that order)
  // decoded picture hash SEI (TAppEncCfg.cpp:1093): 0 none, 1 MD5 of the output picture behind every access unit
  const int hash_sei = (int)opt.geti("SEIDecodedPictureHash", 0);
  // PrintMSSSIM: computed on the device from the pictures the pipeline still holds there (hevcdl_enable_quality); the two MSE keys only print what the PSNR is made of
  // DeviceEntropy 1: the slice data is coded on the device (hevcdl_enable_device_entropy) and the run goes through hevcdl_encode_pictures_stream: records leave HBM only for
  // a record file, pictures only for a reconstruction file, a picture hash or the PSNR of the filtered picture.  Every output is byte for byte that of the run without the key.
  const bool device_entropy = opt.geti("DeviceEntropy", 0) != 0;
  // DeviceReport 1: the squared errors behind the PSNR columns and the digests of SEIDecodedPictureHash come from the device (hevcdl_enable_picture_report), computed where the
  // output picture is; a DeviceEntropy run then fetches pictures for a reconstruction file only.  Stream, reconstruction file and log are those of the run without the key.
  const long device_report_v = opt.geti("DeviceReport", 0);
  if (device_report_v != 0 && device_report_v != 1) opt.errors.push_back("DeviceReport = " + std::to_string(device_report_v) + " is not a value of the key (0 or 1)");
  const bool device_report = device_report_v == 1;
  const bool print_msssim = opt.geti("PrintMSSSIM", 0) != 0, print_frame_mse = opt.geti("PrintFrameMSE", 0) != 0, print_seq_mse = opt.geti("PrintSequenceMSE", 0) != 0;
  for (const char *key : { "LoopFilterBetaOffset_div2", "LoopFilterTcOffset_div2" }) {      // the reference's own range check (TAppEncCfg.cpp xConfirmPara: -6 .. 6)
    const long v = opt.geti(key, 0);
    if (v < -6 || v > 6) opt.errors.push_back(std::string(key) + " = " + std::to_string(v) + " is out of range (-6 .. 6)");
  }
  // DeblockingFilterMetric (TAppEncCfg.cpp:910): 1 = one deblocking offset per picture from the blockiness of its reconstruction, in the slice header; LoopFilterOffsetInPPS
  // (:907) 0 = the slice header repeats the cfg's offsets.  The reference's own condition and text (:2143); mode 2 chains every picture's search to the one before it
  const long dbk_metric = opt.geti("DeblockingFilterMetric", 0), lf_in_pps = opt.geti("LoopFilterOffsetInPPS", 1) != 0;
  if (dbk_metric < 0 || dbk_metric > 2) opt.errors.push_back("DeblockingFilterMetric = " + std::to_string(dbk_metric) + " is not a value of the key (0, 1 or 2)");
  else if (dbk_metric != 0 && (!deblock || lf_in_pps)) opt.errors.push_back("If DeblockingFilterMetric is non-zero then both LoopFilterDisable and LoopFilterOffsetInPPS must be 0");
  else if (dbk_metric == 1 && width > 0 && height > 0 && (width < 64 || height < 64)) opt.errors.push_back("DeblockingFilterMetric = 1 needs a coded picture of at least 64 luma samples in either direction");
  if (hash_sei < 0 || hash_sei > 3) opt.errors.push_back("SEIDecodedPictureHash = " + std::to_string(hash_sei) + " is not a hash of the reference (0 none, 1 MD5, 2 CRC, 3 checksum)");
  // tiles (TAppEncCfg.cpp:1024-1028): uniformly spaced columns x rows or explicit sizes; LFCrossTileBoundaryFlag (default 1) lets the in-loop filters cross tile borders
  const int tile_cols = (int)opt.geti("NumTileColumnsMinus1", 0) + 1, tile_rows = (int)opt.geti("NumTileRowsMinus1", 0) + 1;
  const int tile_uniform = (int)opt.geti("TileUniformSpacing", 0) != 0;
  std::vector<int> tile_cw, tile_rh;               // TileColumnWidthArray / TileRowHeightArray: sizes in CTUs of all but the last column / row
  auto parse_ints = [](const std::string &text, std::vector<int> &out) { std::string t = text; for (char &ch : t) if (ch == ',') ch = ' '; std::istringstream is(t); int v; while (is >> v) out.push_back(v); };
  // WaveFrontSynchro (TAppEncCfg.cpp:975): 1 = entropy_coding_sync_enabled_flag; CTU rows start from the contexts behind the second CTU of the row above and are walked by
  // waves of their own on the device.  The reference refuses the key together with tiles outside the high-throughput profile (TAppEncCfg.cpp xCheckParameter); so does this path.
  const long wavefront = opt.geti("WaveFrontSynchro", 0);
  if (wavefront != 0 && wavefront != 1) opt.errors.push_back("WaveFrontSynchro = " + std::to_string(wavefront) + " is not a value of the key (0 or 1)");
  if (wavefront && tile_cols * tile_rows > 1) opt.errors.push_back("Tiles and entropy-coding-sync (Wavefronts) can not be applied together (as the reference, outside its high-throughput profile)");
  if (tile_cols * tile_rows > 1) {
    if (!tile_uniform) {
      parse_ints(opt.get("TileColumnWidthArray"), tile_cw); parse_ints(opt.get("TileRowHeightArray"), tile_rh);
      if ((int)tile_cw.size() < tile_cols - 1 || (int)tile_rh.size() < tile_rows - 1 || tile_cols > 20 || tile_rows > 22)
        opt.errors.push_back("TileUniformSpacing = 0 needs TileColumnWidthArray / TileRowHeightArray with a size for every tile column / row but the last");
    }
  }
  // Slices (TAppEncCfg.cpp:1008-1017): SliceMode 1 = SliceArgument CTUs a slice (whole CTU rows only on this path), 3 = SliceArgument tiles a slice; SliceArgument and
  // LFCrossSliceBoundaryFlag are read only then (the default cfg carries SliceArgument 1500 beside SliceMode 0).  What hevcdl_create refuses arrives with its reason.
  const long slice_mode = opt.geti("SliceMode", 0), slice_arg = slice_mode ? opt.geti("SliceArgument", 0) : 0, lf_slices = slice_mode ? opt.geti("LFCrossSliceBoundaryFlag", 1) != 0 : 1;
  if (slice_mode < 0 || slice_mode > 3) opt.errors.push_back("SliceMode = " + std::to_string(slice_mode) + " is not a value of the key (0, 1 or 3; 2 is not implemented by this path)");
  else if (slice_mode == 2) opt.errors.push_back("SliceMode = 2 (slices by bytes) is not implemented by this path: the slice borders would depend on the coded bytes");
  else if (slice_mode == 1 && (tile_cols * tile_rows > 1 || wavefront)) opt.errors.push_back("SliceMode = 1 together with tiles or WaveFrontSynchro is not implemented by this path");
  else if (slice_mode == 1 && width > 0 && height > 0 && (slice_arg < 1 || slice_arg % ((width + 63) / 64) != 0 || (((height + 63) / 64) + slice_arg / ((width + 63) / 64) - 1) / (slice_arg / ((width + 63) / 64)) > 22))
    opt.errors.push_back("SliceMode = 1 needs a SliceArgument that is a positive multiple of the picture's width in CTUs (" + std::to_string((width + 63) / 64) + ") and gives at most 22 slices a picture: only slices of whole CTU rows are implemented");
  else if (slice_mode == 3 && (tile_cols * tile_rows == 1 || slice_arg < 1)) opt.errors.push_back("SliceMode = 3 (slices of whole tiles) needs tiles and a SliceArgument of at least 1");
  else if (slice_mode == 3 && slice_arg > 1 && opt.geti("LFCrossTileBoundaryFlag", 1) != 0 && !lf_slices)
    opt.errors.push_back("SliceMode = 3 with more than one tile a slice, LFCrossTileBoundaryFlag = 1 and LFCrossSliceBoundaryFlag = 0 is not implemented by this path (the in-loop filters have one flag for all tile borders)");
  else if (slice_mode != 0 && dbk_metric != 0) opt.errors.push_back("slices together with DeblockingFilterMetric are not implemented by this path");
  // Dependent slice segments (TAppEncCfg.cpp:942-943): SliceSegmentMode 1 = SliceSegmentArgument CTUs a segment (whole rows of a WaveFrontSynchro picture on this path),
  // 3 = SliceSegmentArgument tiles a segment; the argument is read only then.  What hevcdl_create refuses is refused here in its words (csrc/slice_grid.h).
  const long seg_mode = opt.geti("SliceSegmentMode", 0), seg_arg = seg_mode ? opt.geti("SliceSegmentArgument", 0) : 0;
  if (seg_mode != 0 && width > 0 && height > 0) {
    hevcdl_config probe; memset(&probe, 0, sizeof probe);
    probe.width = width; probe.height = height; probe.tile_columns = tile_cols; probe.tile_rows = tile_rows; probe.wavefront = wavefront ? 1 : 0; probe.deblocking_metric = (int)dbk_metric;
    probe.slice_mode = (int)slice_mode; probe.slice_segment_mode = (int)seg_mode; probe.slice_segment_argument = (int)seg_arg;
    const char *why = "";
    if (hevcdl_segment_keys(&probe, &why) != HEVCDL_OK) opt.errors.push_back("SliceSegmentMode = " + std::to_string(seg_mode) + ", SliceSegmentArgument = " + std::to_string(seg_arg) + ": " + why);
  }
  // DeltaQpRD (TAppEncCfg.cpp:897, "-dqr"): every picture is decided at QP, QP - 1, QP + 1, ... QP + N and the cheapest candidate is kept (TEncSlice::precompressSlice).
  // What hevcdl_create refuses is refused here in its words (csrc/qp_rd.h).
  const long delta_qp_rd = opt.geti("DeltaQpRD", 0);
  if (delta_qp_rd != 0) {
    hevcdl_config probe; memset(&probe, 0, sizeof probe);
    probe.qp = qp; probe.bit_depth = bit_depth; probe.deblocking_metric = (int)dbk_metric; probe.slice_mode = (int)slice_mode; probe.slice_segment_mode = (int)seg_mode; probe.delta_qp_rd = (int)delta_qp_rd;
    const char *why = "";
    if (delta_qp_rd < -1000 || delta_qp_rd > 1000) probe.delta_qp_rd = -1;
    if (hevcdl_qp_rd_keys(&probe, &why) != HEVCDL_OK) opt.errors.push_back("DeltaQpRD = " + std::to_string(delta_qp_rd) + ": " + why);
  }
  // A QP per picture.  dQPFile ("-m"), QPIncrementFrame ("-qpif"), IntraQPOffset: qp[poc] = Clip3(-QpBDOffset, 51, QP + dqp[poc] + IntraQPOffset); LambdaModifierI
  // (its first value: there is one temporal layer), else LambdaModifier0: the factor on every picture's lambda.  The rule and what is refused: csrc/frame_qp.h.
  const std::string dqp_file = native_path(opt.get("dQPFile"));
  const bool qpif_present = opt.v.count("QPIncrementFrame") && !opt.get("QPIncrementFrame").empty();
  const long qpif = qpif_present ? opt.geti("QPIncrementFrame", 0) : -1, intra_qp_offset = opt.geti("IntraQPOffset", 0);
  double lambda_modifier = 1.0;
  if (opt.v.count("LambdaModifierI") && !opt.get("LambdaModifierI").empty()) lambda_modifier = atof(opt.get("LambdaModifierI").c_str());
  else if (opt.v.count("LambdaModifier0")) lambda_modifier = atof(opt.get("LambdaModifier0").c_str());
  if (qpif_present && qpif < 0) opt.errors.push_back("QPIncrementFrame = " + std::to_string(qpif) + " is not a source frame number");
  const bool frame_qp_keys = !dqp_file.empty() || qpif_present || intra_qp_offset != 0;
  // the QPs of pictures 0 .. n - 1 of the sequence; false with the sentence in `why`
  auto sequence_qps = [&](long n, std::vector<int> &qps, std::string &why) -> bool {
    std::vector<int> dqp((size_t)std::max<long>(n, 0));
    hevcdl_dqp_increment(dqp.data(), (int)dqp.size(), qpif_present && qpif >= 0, (unsigned)std::max<long>(qpif, 0), (unsigned)std::max<long>(frame_skip, 0), (unsigned)std::max<long>(ts_ratio, 1));
    if (!dqp_file.empty()) {
      const int got = hevcdl_dqp_read_file(dqp_file.c_str(), dqp.data(), (int)dqp.size());
      if (got == -1) { why = "dQPFile '" + dqp_file + "' cannot be opened"; return false; }
      if (got < 0) { why = "dQPFile '" + dqp_file + "' must hold whitespace-separated integers of -64 .. 64, one a POC"; return false; }
    }
    qps.resize(dqp.size());
    for (size_t i = 0; i < dqp.size(); i++) qps[i] = hevcdl_frame_qp_of(qp, dqp[i], (int)intra_qp_offset, bit_depth);
    return true;
  };
  std::vector<int> seq_qps;
  if (frame_qp_keys || lambda_modifier != 1.0) {
    hevcdl_config probe; memset(&probe, 0, sizeof probe);
    probe.qp = qp; probe.bit_depth = bit_depth; probe.deblocking_metric = (int)dbk_metric; probe.delta_qp_rd = (int)delta_qp_rd;
    std::string why;
    const long n_known = std::max<long>(1, (n_frames + std::max<long>(ts_ratio, 1) - 1) / std::max<long>(ts_ratio, 1));      // (FramesToBeEncoded 0: the file's length decides below; one picture shows every refusal but a value's)
    if (frame_qp_keys && !sequence_qps(n_known, seq_qps, why)) opt.errors.push_back(why);
    else {
      const char *w = "";
      if (hevcdl_frame_qp_keys(&probe, frame_qp_keys ? seq_qps.data() : nullptr, frame_qp_keys ? (int)seq_qps.size() : 0, lambda_modifier, &w) != HEVCDL_OK) opt.errors.push_back(w);
    }
  }
  char qp_line[160];      // TAppEncCfg.cpp:2927-2933
  if (qpif_present) snprintf(qp_line, sizeof qp_line, "QP                                     : %d (incrementing internal QP at source frame %ld)", qp, qpif);
  else snprintf(qp_line, sizeof qp_line, "QP                                     : %d", qp);
  if (opt.v.count("PrintConfig")) {
    printf("{\"DeltaQpRD\": %ld, ", delta_qp_rd);
    printf("\"QPLine\": \"%s\", \"dQPFile\": \"%s\", \"QPIncrementFrame\": %ld, \"IntraQPOffset\": %ld, \"LambdaModifier\": %.17g, \"FrameQPs\": [", qp_line, json_escape(dqp_file).c_str(), qpif, intra_qp_offset, lambda_modifier);
    for (size_t i = 0; i < seq_qps.size(); i++) printf("%s%d", i ? ", " : "", seq_qps[i]);
    printf("], ");
    printf("\"SliceMode\": %ld, \"SliceArgument\": %ld, \"LFCrossSliceBoundaryFlag\": %ld, \"SliceSegmentMode\": %ld, \"SliceSegmentArgument\": %ld, ", slice_mode, slice_arg, lf_slices, seg_mode, seg_arg);
    printf("\"InputFile\": \"%s\", \"ReconFile\": \"%s\", \"SourceWidth\": %d, \"SourceHeight\": %d, \"QP\": %d, \"FrameSkip\": %ld, \"FramesToBeEncoded\": %ld, "
           "\"FrameRate\": %g, \"LabelDir\": \"%s\", \"CnnInput\": \"%s\", \"BitstreamFile\": \"%s\", \"level_idc\": %d, \"tiles\": [%d, %d], \"bit_depth\": %d, "
           "\"ConformanceWindowMode\": %d, \"HorizontalPadding\": %d, \"VerticalPadding\": %d, \"InputBitDepth\": %d, \"InternalBitDepth\": %d, \"OutputBitDepth\": %d, \"coded_size\": [%d, %d], "
           "\"InputChromaFormat\": %d, \"ChromaFormatIDC\": %d, \"Input ChromaFormatIDC\": \"4:%c:%c\", \"Output (internal) ChromaFormatIDC\": \"4:2:0\", \"InputColourSpaceConvert\": \"%s\", "
           "\"OutputInternalColourSpace\": %d, \"SNRInternalColourSpace\": %d, \"ConfWin\": [%d, %d, %d, %d], \"TemporalSubsampleRatio\": %ld, \"stage_keys\": [", json_escape(input).c_str(), json_escape(recon_path).c_str(), src_w, src_h, qp,
           frame_skip, n_frames, fps, json_escape(label_dir).c_str(), cnn_input.c_str(), json_escape(bitstream_path).c_str(), level_idc, tile_cols, tile_rows, bit_depth,
           conf_mode, pad_x, pad_y, in_bd, bit_depth, out_bd, width, height,
           in_cf, cf_idc == 0 ? in_cf : cf_idc, in_cf == 400 ? '0' : (in_cf == 444 ? '4' : '2'), in_cf == 400 ? '0' : (in_cf == 420 ? '0' : (in_cf == 422 ? '2' : '4')), colour_space ? "YCbCrtoYCrCb" : "UNCHANGED",
           out_internal_cs, snr_internal_cs, win_l, win_r, win_t, win_b, ts_ratio);
    for (size_t i = 0; i < stage_keys.size(); i++) printf("%s\"%s\"", i ? ", " : "", stage_keys[i].c_str());
    printf("], \"errors\": [");
    for (size_t i = 0; i < opt.errors.size(); i++) printf("%s\"%s\"", i ? ", " : "", json_escape(opt.errors[i]).c_str());
    printf("]}\n");
    return opt.errors.empty() ? 0 : 2;
  }
  if (input.empty()) opt.errors.push_back("InputFile (-i) is required");
  if (width <= 0 || height <= 0) opt.errors.push_back("SourceWidth / SourceHeight (-wdt / -hgt) are required");
  if (cnn_input != "rgb601" && cnn_input != "luma") opt.errors.push_back("CnnInput must be rgb601 or luma");
  const std::string bn_mode = opt.get("BnMode", "reference");        // reference: training-mode BatchNorm as use_model.py runs it; eval: running statistics
  if (bn_mode != "reference" && bn_mode != "eval") opt.errors.push_back("BnMode must be reference or eval");
  if (!opt.errors.empty()) { for (const auto &e : opt.errors) fprintf(stderr, "Error: %s\n", e.c_str()); return 2; }

  const size_t frame_bytes = hevcdl_frame_bytes_bd(width, height, bit_depth);      // a coded picture
  hevcdl_source_format fmt; memset(&fmt, 0, sizeof fmt);
  fmt.struct_size = sizeof fmt; fmt.source_width = src_w; fmt.source_height = src_h; fmt.input_bit_depth = in_bd; fmt.output_bit_depth = out_bd;
  fmt.chroma_format = in_cf == 420 ? 0 : in_cf; fmt.colour_space = colour_space; fmt.output_internal_colour_space = out_internal_cs; fmt.snr_internal_colour_space = snr_internal_cs;
  fmt.conf_win_left = win_l; fmt.conf_win_right = win_r; fmt.conf_win_top = win_t; fmt.conf_win_bottom = win_b;
  const size_t src_frame_bytes = use_fmt ? hevcdl_source_frame_bytes(&fmt) : frame_bytes, out_frame_bytes = use_fmt ? hevcdl_output_frame_bytes(&fmt) : frame_bytes;      // a frame of the input file / of the reconstruction file
  if (src_frame_bytes == 0) { fprintf(stderr, "Error: unsupported source size / bit depths\n"); return 2; }
  FILE *fin = fopen(input.c_str(), "rb");
  if (!fin) { fprintf(stderr, "Error: cannot open input file '%s'\n", input.c_str()); return 2; }
  fseek(fin, 0, SEEK_END); const long long fsize = ftell(fin);
  fclose(fin);
  const long avail = (long)(fsize / (long long)src_frame_bytes) - frame_skip;
  if (avail <= 0) { fprintf(stderr, "Error: input holds no frame after FrameSkip\n"); return 2; }
  if (n_frames <= 0 || n_frames > avail) n_frames = avail;                    // TAppEncTop: stops at end of file
  n_frames = (n_frames + ts_ratio - 1) / ts_ratio;                            // source frames -> pictures: picture k is source frame FrameSkip + k * ratio; POCs are consecutive
  if (frame_qp_keys) { // the QP of every picture of the sequence, once; every shard and batch takes its slice
    std::string why; const char *w = "";
    hevcdl_config probe; memset(&probe, 0, sizeof probe); probe.bit_depth = bit_depth;
    if (!sequence_qps(n_frames, seq_qps, why)) { fprintf(stderr, "Error: %s\n", why.c_str()); return 2; }
    if (hevcdl_frame_qp_keys(&probe, seq_qps.data(), (int)seq_qps.size(), lambda_modifier, &w) != HEVCDL_OK) { fprintf(stderr, "Error: %s\n", w); return 2; }
  }
  // Devices.  --Device d (default 0): one device.  --Devices 0-7 | 0,2,5 | --NumDevices N: the frames of the job in contiguous blocks, one block, one host thread and
  // one context per entry (the app loop of TAppEncTop.cpp:568-691 once per block; -fs / -f of TAppEncCfg.cpp:786,788 are what a block is); an entry may repeat a
  // device (two contexts share it: the contexts then never wait on each other, HEVCDL_EXEC_NO_UNIT_HANDOVER).
  std::vector<int> devices;
  if (opt.v.count("Devices")) {
    std::string t = opt.get("Devices"); for (char &ch : t) if (ch == ',') ch = ' ';
    std::istringstream is(t); std::string tok;
    while (is >> tok) { const size_t d = tok.find('-'); if (d != std::string::npos && d > 0) { for (int v = atoi(tok.substr(0, d).c_str()); v <= atoi(tok.substr(d + 1).c_str()); v++) devices.push_back(v); } else devices.push_back(atoi(tok.c_str())); }
  } else if (opt.v.count("NumDevices")) { for (int v = 0; v < (int)opt.geti("NumDevices", 1); v++) devices.push_back(v); }
  else devices.push_back((int)opt.geti("Device", 0));
  if (dbk_metric == 2 && devices.size() > 1) { fprintf(stderr, "Error: DeblockingFilterMetric = 2 on %zu devices: every picture's search window lies round the choice of the picture before it, so the pictures of a sequence are one chain and cannot be dealt to devices; name one device\n", devices.size()); return 2; }
  if (devices.empty() || devices.size() > 64) { fprintf(stderr, "Error: Devices / NumDevices must name 1..64 devices\n"); return 2; }
  const int n_shards = (int)std::min<long>((long)devices.size(), n_frames);
  const bool multi = devices.size() > 1;
  bool shared_device = false;
  for (size_t i = 0; i < devices.size(); i++) for (size_t j = 0; j < i; j++) if (devices[i] == devices[j]) shared_device = true;
  const long per_shard = (n_frames + n_shards - 1) / n_shards;                // the largest block: sharding.shard_frames deals contiguous blocks [i * n / shards, (i + 1) * n / shards), none empty
  // Pictures per device call.  A frame is a serial chain of CTUs: a call costs about the same from 1 to ~250 pictures and grows slowly beyond (the decision kernel
  // keeps one workgroup per CU busy with 1..8 pictures), so the default is a device's whole share, bounded by the 2048 (picture, tile) units the GPU holds, by 24 GiB
  // of originals on the host and by the DEVICE's free memory: a picture of a call occupies 3 frame buffers (original, reconstruction, filtered picture), its CTU
  // records, labels / logits and SAO parameters in HBM (hevcdl_create is retried with half the batch when the device refuses).  The results of a call come back chunk by
  // chunk (hevcdl_encode_pictures_chunked): the host never holds more than the originals of a batch and two chunks of results.  Several device calls: equal shares.
  const int ctus = hevcdl_ctus_per_frame(width, height);
  const long per_picture_dev = 3 * (long)frame_bytes + (long)ctus * ((long)sizeof(hevcdl_ctu_record) + 16 + 256 + 3 * 140) + (2L << 20);
  long dev_cap = 2048;
  { size_t free_b = 0, total_b = 0;       // the smallest free memory over the devices named: every shard's batch is sized from it
    for (size_t i = 0; i < devices.size(); i++) { size_t f = 0, t = 0; if (hevcdl_device_memory(devices[i], &f, &t) == HEVCDL_OK && f > 0 && (free_b == 0 || f < free_b)) { free_b = f; total_b = t; } }
    const size_t workspace = (size_t)4400 << 20;        // the decision kernel's workspace: up to 1.6 MB x 10 waves x 256 workgroups per context (hevcdl_reserve_workspace)
    if (free_b > 0) { double mine = (double)free_b * 0.8 / (shared_device ? (double)devices.size() : 1.0);       // (contexts that share a device share its memory)
      if (mine > 2.0 * (double)workspace) mine -= (double)workspace;
      dev_cap = std::max<long>(1, (long)mine / per_picture_dev); } }
  const long units_per_picture = slice_mode == 1 ? (((height + 63) / 64) * (long)((width + 63) / 64) + slice_arg - 1) / slice_arg : (long)tile_cols * tile_rows;      // independent units of the decision launch: tiles, or row slices
  const long auto_batch = std::max<long>(1, std::min<long>(std::min<long>(2048 / units_per_picture, dev_cap), (24L << 30) / (long)frame_bytes));
  const long even_batch = (per_shard + ((per_shard + auto_batch - 1) / auto_batch) - 1) / ((per_shard + auto_batch - 1) / auto_batch);
  int batch = (int)std::min<long>(per_shard, std::max<long>(1, opt.geti("BatchFrames", even_batch)));

  hevcdl_config cfg;
  hevcdl_status st = hevcdl_config_default_bd(&cfg, width, height, qp, bit_depth);
  if (st != HEVCDL_OK) { fprintf(stderr, "Error: unsupported picture size / QP (status %d)\n", (int)st); return 2; }
  cfg.tile_columns = tile_cols; cfg.tile_rows = tile_rows; cfg.wavefront = (int)wavefront;
  if (tile_cols * tile_rows > 1) {
    cfg.tile_uniform_spacing = tile_uniform; cfg.lf_across_tiles = opt.geti("LFCrossTileBoundaryFlag", 1) != 0;
    if (!tile_uniform) { for (int i = 0; i < tile_cols - 1; i++) cfg.tile_column_width[i] = tile_cw[i]; for (int i = 0; i < tile_rows - 1; i++) cfg.tile_row_height[i] = tile_rh[i]; }
  }
  // tool switches of the cfg (TAppEncCfg.cpp:900-901,917-918,950,978,1007; encoder_intra_main.cfg:37-38,53-54): defaults as the reference's
  uint32_t tools = HEVCDL_TOOLS_REFERENCE;
  if (opt.geti("RDOQ", 1) == 0) tools &= ~HEVCDL_TOOL_RDOQ;
  if (opt.geti("RDOQTS", 1) == 0) tools &= ~HEVCDL_TOOL_RDOQTS;
  if (opt.geti("TransformSkip", 1) == 0) tools &= ~HEVCDL_TOOL_TSKIP;
  if (opt.geti("TransformSkipFast", 1) == 0) tools &= ~HEVCDL_TOOL_TSKIP_FAST;
  if (opt.geti("SignHideFlag", 1) == 0) tools &= ~HEVCDL_TOOL_SIGN_HIDE;
  if (opt.geti("StrongIntraSmoothing", 1) == 0) tools &= ~HEVCDL_TOOL_STRONG_INTRA;
  if (opt.geti("FastUDIUseMPMEnabled", 1) == 0) tools &= ~HEVCDL_TOOL_FAST_UDI_MPM;
  cfg.tools = tools;
  cfg.lf_beta_offset_div2 = (int)opt.geti("LoopFilterBetaOffset_div2", 0); cfg.lf_tc_offset_div2 = (int)opt.geti("LoopFilterTcOffset_div2", 0);      // -6 .. 6 (hevcdl_create checks)
  cfg.deblocking_metric = (int)dbk_metric; cfg.lf_offset_in_pps = (int)lf_in_pps;
  cfg.slice_mode = (int)slice_mode; cfg.slice_argument = (int)slice_arg; cfg.lf_across_slices = (int)lf_slices;
  cfg.slice_segment_mode = (int)seg_mode; cfg.slice_segment_argument = (int)seg_arg;
  cfg.delta_qp_rd = (int)delta_qp_rd;
  cfg.cnn_input = cnn_input == "luma" ? HEVCDL_CNN_INPUT_LUMA : HEVCDL_CNN_INPUT_RGB601;
  cfg.bn_mode = bn_mode == "eval" ? HEVCDL_BN_EVAL : HEVCDL_BN_REFERENCE;
  if (shared_device) cfg.exec_flags |= HEVCDL_EXEC_NO_UNIT_HANDOVER;
  std::string wpath = opt.get("Weights");
  if (wpath.empty()) { // next to the library: <pkg>/weights/hevc_encoder_model.f32, this binary lives in <pkg>/bin
    std::string self = argv[0]; const size_t s1 = self.find_last_of('/'); self = s1 == std::string::npos ? "." : self.substr(0, s1);
    wpath = self + "/../weights/hevc_encoder_model.f32";
  }
  std::vector<float> weights(HEVCDL_WEIGHT_FLOATS);
  { FILE *fw = fopen(wpath.c_str(), "rb");
    if (!fw || fread(weights.data(), sizeof(float), weights.size(), fw) != weights.size()) { fprintf(stderr, "Error: cannot read %d weights from '%s'\n", (int)HEVCDL_WEIGHT_FLOATS, wpath.c_str()); return 2; }
    fclose(fw); }

  // one block of frames per device entry
  struct PicOut { std::vector<uint8_t> bytes; size_t au_len = 0; char md5_text[128]; unsigned long long sse[3]; hevcdl_status st = HEVCDL_OK; };
  struct Shard {
    int dev = 0; long f_lo = 0, f_hi = 0; hevcdl_ctx *ctx = nullptr; int batch = 1; int rc = 0;
    double t_read = 0, t_dev = 0, t_host = 0, t_write = 0;
    std::vector<unsigned long long> rows;       // per coded picture: { poc, bits, sse Y, sse U, sse V, ctus, encode ns, device, slice QP }  (what the devices gather); PrintMSSSIM: + the three MS-SSIM doubles' bit patterns
    std::vector<std::vector<uint8_t>> aus;      // multi-device runs: the access units (+ hash SEI) of the block, written out in POC order at the end
    std::vector<std::string> md5;
  };
  const int ROW = print_msssim ? 12 : 9;
  std::vector<Shard> shards(n_shards);
  for (int i = 0; i < n_shards; i++) { shards[i].dev = devices[i]; shards[i].f_lo = (long)i * n_frames / n_shards; shards[i].f_hi = (long)(i + 1) * n_frames / n_shards; }
  for (int i = 0; i < n_shards; i++) { // contexts: created one after the other (a refused allocation halves the batch of every shard)
    for (;;) {
      cfg.max_frames = batch; cfg.device = shards[i].dev;
      st = hevcdl_create(&cfg, weights.data(), weights.size(), &shards[i].ctx);
      // the decision kernel's workspace (up to 4.3 GB) is otherwise allocated by the first launch: reserved here, a lack of memory is met by the retry below
      bool ws_oom = false;
      if (st == HEVCDL_OK && (st = hevcdl_reserve_workspace(shards[i].ctx)) != HEVCDL_OK) { ws_oom = st == HEVCDL_ERR_OOM; hevcdl_destroy(shards[i].ctx); shards[i].ctx = nullptr; }
      // PrintMSSSIM: the quality pass's workspace (pyramids of up to 16 pictures) is reserved by the switch; a refusal halves the batch like any other
      if (st == HEVCDL_OK && print_msssim && (st = hevcdl_enable_quality(shards[i].ctx, 1)) != HEVCDL_OK) { hevcdl_destroy(shards[i].ctx); shards[i].ctx = nullptr; }
      // DeviceEntropy: the sub-stream regions and the packed buffer are reserved by the switch as well
      if (st == HEVCDL_OK && device_entropy && (st = hevcdl_enable_device_entropy(shards[i].ctx, 1)) != HEVCDL_OK) { hevcdl_destroy(shards[i].ctx); shards[i].ctx = nullptr; }
      // DeviceReport: records and partials of a batch (a few KB a picture)
      if (st == HEVCDL_OK && device_report && (st = hevcdl_enable_picture_report(shards[i].ctx, 1, hash_sei)) != HEVCDL_OK) { hevcdl_destroy(shards[i].ctx); shards[i].ctx = nullptr; }
      // a file that is not in the codec's format: the upload buffer of source-format frames and the window crops of a padded picture
      if (st == HEVCDL_OK && use_fmt && (st = hevcdl_set_source_format(shards[i].ctx, &fmt)) != HEVCDL_OK) { hevcdl_destroy(shards[i].ctx); shards[i].ctx = nullptr; }
      // a QP per picture: the modifier once, the first batch's slice of the list in front of the reservation so that the sorted sets are part of it (every batch sets its own below)
      if (st == HEVCDL_OK && lambda_modifier != 1.0 && (st = hevcdl_set_lambda_modifier(shards[i].ctx, lambda_modifier)) != HEVCDL_OK) { fprintf(stderr, "Error: %s\n", hevcdl_last_error(shards[i].ctx)); return 2; }
      if (st == HEVCDL_OK && frame_qp_keys) {
        const long lo = shards[i].f_lo, cnt = std::min<long>(batch, shards[i].f_hi - lo);
        if ((st = hevcdl_set_frame_qps(shards[i].ctx, seq_qps.data() + lo, (int)cnt)) != HEVCDL_OK) { fprintf(stderr, "Error: %s\n", hevcdl_last_error(shards[i].ctx)); return 2; }
        if ((st = hevcdl_reserve_workspace(shards[i].ctx)) != HEVCDL_OK) { hevcdl_destroy(shards[i].ctx); shards[i].ctx = nullptr; }
      }
      if (st == HEVCDL_ERR_OOM && ws_oom) {
        // the workspace is sized by the device's CUs, not by the batch: a smaller batch does not shrink it.  What does: the independent launch form (a block per wave of
        // the context's own frames instead of every CU's workgroup), then the eight-wave build
        if (!(cfg.exec_flags & HEVCDL_EXEC_NO_UNIT_HANDOVER)) cfg.exec_flags |= HEVCDL_EXEC_NO_UNIT_HANDOVER;
        else if (!(cfg.exec_flags & HEVCDL_EXEC_RD_NARROW)) cfg.exec_flags = (cfg.exec_flags & ~HEVCDL_EXEC_RD_WIDE) | HEVCDL_EXEC_RD_NARROW;
        else { fprintf(stderr, "Error: device %d has no memory for the decision kernel's workspace (1.6 MB per wave of a launch) even in the independent launch form\n", shards[i].dev); return 3; }
        fprintf(stderr, "device %d: not enough memory for the decision kernel's workspace, retrying with exec_flags %d\n", shards[i].dev, (int)cfg.exec_flags);
        for (int j = 0; j < i; j++) { hevcdl_destroy(shards[j].ctx); shards[j].ctx = nullptr; }
        i = -1; break;
      }
      if (st != HEVCDL_ERR_OOM || batch == 1) break;
      batch = (batch + 1) / 2;
      fprintf(stderr, "device %d: not enough memory for the batch, retrying with %d pictures per call\n", shards[i].dev, batch);
      for (int j = 0; j < i; j++) { hevcdl_destroy(shards[j].ctx); shards[j].ctx = nullptr; }
      i = -1; break;
    }
    if (i < 0) continue;
    if (st != HEVCDL_OK && hevcdl_create_error()[0]) { fprintf(stderr, "Error: %s\n", hevcdl_create_error()); return 2; }
    if (st == HEVCDL_ERR_INVALID_ARG) { fprintf(stderr, "Error: hevcdl_create rejected the configuration as invalid (e.g. tiles, which must be at least 4 CTUs wide and 1 CTU high: TComPicSym.cpp:380-392)\n"); return 2; }
    if (st != HEVCDL_OK) { fprintf(stderr, "Error: hevcdl_create failed on device %d with status %d (no GPU / unsupported configuration); there is no CPU path\n", shards[i].dev, (int)st); return 3; }
  }
  const double t_setup = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_main0).count();      // options, weights, contexts, the decision kernel's workspace
  const int chunk = (int)std::max<long>(1, std::min<long>(batch, opt.geti("ChunkFrames", 48)));

  if (conf_mode == 3 && !(win_l | win_r | win_t | win_b)) fprintf(stderr, "Warning: Conformance window enabled, but all conformance window parameters set to zero\n");
  if (conf_mode == 3 && (pad_x || pad_y)) fprintf(stderr, "Warning: Conformance window enabled, padding parameters will be ignored\n");
  if (use_fmt) printf("Source %dx%d at %d bits -> coded %dx%d at %d bits (conformance window right %d, bottom %d), output at %d bits\n", src_w, src_h, in_bd, width, height, bit_depth, conf_mode == 3 ? win_r : width - src_w, conf_mode == 3 ? win_b : height - src_h, out_bd);
  if (in_cf != 420 || colour_space || conf_mode == 3 || ts_ratio > 1) { // TAppEncTop::printChromaFormat, and what else of the file's layout is in force
    printf("%43s  4:%c:%c\n%43s  4:2:0\n\n", "Input ChromaFormatIDC = ", in_cf == 400 ? '0' : (in_cf == 444 ? '4' : '2'), in_cf == 400 ? '0' : (in_cf == 420 ? '0' : (in_cf == 422 ? '2' : '4')), "Output (internal) ChromaFormatIDC = ");
    printf("File layout: colour space %s, window left %d right %d top %d bottom %d, every %ld. source frame\n", colour_space ? "YCbCrtoYCrCb" : "UNCHANGED", win_l, win_r, win_t, win_b, ts_ratio);
  }
  if (qpif_present) printf("%s\n", qp_line);
  printf("HEVC-DL MI355X path: %dx%d  QP %d  frames %ld (skip %ld)  batch %d  labels: %s\n", width, height, qp, n_frames, frame_skip, batch,
         label_dir.empty() ? (cnn_input == "luma" ? "on-device CNN (luma input)" : "on-device CNN (BT.601 RGB input)") : ("files under " + label_dir).c_str());
  if (multi) {
    printf("Devices:");
    for (int i = 0; i < n_shards; i++) printf(" %d (frames %ld..%ld)", shards[i].dev, shards[i].f_lo, shards[i].f_hi - 1);
    printf("\n");
  }
  if (!stage_keys.empty()) {
    printf("Accepted without effect on this path:");
    for (const auto &k : stage_keys) printf(" %s", k.c_str());
    printf("\n");
  }
  FILE *frec = recon_path.empty() ? nullptr : fopen(recon_path.c_str(), "wb");
  if (!recon_path.empty() && !frec) { fprintf(stderr, "Error: cannot open reconstruction file '%s'\n", recon_path.c_str()); return 2; }
  const std::string record_path = native_path(opt.get("RecordFile"));
  FILE *frecords = record_path.empty() ? nullptr : fopen(record_path.c_str(), "wb");
  FILE *fbits = bitstream_path.empty() ? nullptr : fopen(bitstream_path.c_str(), "wb");
  if (!bitstream_path.empty() && !fbits) { fprintf(stderr, "Error: cannot open bitstream file '%s'\n", bitstream_path.c_str()); return 2; }
  hevcdl_stream_config scfg; hevcdl_stream_config_default(&scfg, width, height, qp); scfg.level_idc = level_idc; scfg.sao_enabled = sao; scfg.tile_columns = tile_cols; scfg.tile_rows = tile_rows; scfg.bit_depth = bit_depth; scfg.wavefront = (int)wavefront;
  scfg.rewrite_param_sets = opt.geti("ReWriteParamSetsFlag", 1) != 0;
  scfg.tools = cfg.tools; scfg.lf_beta_offset_div2 = cfg.lf_beta_offset_div2; scfg.lf_tc_offset_div2 = cfg.lf_tc_offset_div2; scfg.loop_filter_disable = deblock ? 0 : 1;
  scfg.lf_across_tiles = cfg.lf_across_tiles; scfg.tile_uniform_spacing = cfg.tile_uniform_spacing; memcpy(scfg.tile_column_width, cfg.tile_column_width, sizeof scfg.tile_column_width); memcpy(scfg.tile_row_height, cfg.tile_row_height, sizeof scfg.tile_row_height);
  scfg.conf_win_right = width - src_w; scfg.conf_win_bottom = height - src_h;
  const hevcdl_slice_layout slices = { (int)slice_mode, (int)slice_arg, (int)lf_slices };      // NAL units, slice headers and the PPS's across-slices flag (mode 0: one slice, as ever)
  const hevcdl_segment_layout segments = { (int)seg_mode, (int)seg_arg };      // a NAL unit per dependent slice segment (mode 0: none)
  if (conf_mode == 3) { scfg.conf_win_left = win_l; scfg.conf_win_right = win_r; scfg.conf_win_top = win_t; scfg.conf_win_bottom = win_b; }      // PSNR, the hash and the digests stay over the whole coded picture (no padding: m_aiPad is 0)
  const double ny = (double)src_w * src_h, nc = ny / 4;      // PSNR, MSE and MS-SSIM are taken over the picture without the padding (TEncGOP.cpp:2302-2303, 2375-2376)
  double sum_bits = 0, sum_psnr[3] = { 0, 0, 0 }, sum_mse[3] = { 0, 0, 0 }, sum_msssim[3] = { 0, 0, 0 }; long done = 0;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
  // host threads for the per-picture work: the CPUs this process may really use (a container's CPU quota is often far below the node's thread count)
  unsigned cpus = std::max(1u, std::thread::hardware_concurrency());
  { FILE *fq = fopen("/sys/fs/cgroup/cpu.max", "r"); long long q = 0, per = 0; char qs[32];
    if (fq) { if (fscanf(fq, "%31s %lld", qs, &per) == 2 && strcmp(qs, "max") != 0 && per > 0) { q = atoll(qs); if (q > 0) cpus = (unsigned)std::max<long long>(1, std::min<long long>(cpus, q / per)); } fclose(fq); } }
  const int max_threads = (int)std::max(1u, std::min(cpus, 64u) / (unsigned)n_shards);
  const double maxval = (double)(255 << (bit_depth - 8));
  // one picture's log line and its share of the summary (TEncGOP.cpp:2500-2541; PSNR from the squared error as TEncGOP.cpp:2391-2394)
  // msssim_bits: the picture's three MS-SSIM values as bit patterns (PrintMSSSIM), or null
  // pic_qp: the slice QP the picture was coded with (the cfg's, or with DeltaQpRD the candidate kept for it)
  auto log_picture = [&](long poc, int pic_qp, unsigned long long bits, const unsigned long long *sse, double et, const char *md5_text, const unsigned long long *msssim_bits) {
    const double p[3] = { psnr_of(sse[0], ny, maxval), psnr_of(sse[1], nc, maxval), psnr_of(sse[2], nc, maxval) };
    if (!print_msssim && !print_frame_mse)
      printf("POC %4ld TId: %1d ( %c-SLICE, QP %d ) %10llu bits [Y %6.4lf dB    U %6.4lf dB    V %6.4lf dB] [ET %5.0f ]%s\n", poc, 0, 'I', pic_qp, bits, p[0], p[1], p[2], et, md5_text);
    else { // the groups of TEncGOP.cpp:2522-2537 between the PSNR group and [ET
      printf("POC %4ld TId: %1d ( %c-SLICE, QP %d ) %10llu bits [Y %6.4lf dB    U %6.4lf dB    V %6.4lf dB]", poc, 0, 'I', pic_qp, bits, p[0], p[1], p[2]);
      if (print_msssim) {
        double m[3]; memcpy(m, msssim_bits, sizeof m);
        printf(" [MS-SSIM Y %1.6lf    U %1.6lf    V %1.6lf]", m[0], m[1], m[2]);
        for (int c = 0; c < 3; c++) sum_msssim[c] += m[c];
      }
      if (print_frame_mse) printf(" [Y MSE %6.4lf  U MSE %6.4lf  V MSE %6.4lf]", (double)sse[0] / ny, (double)sse[1] / nc, (double)sse[2] / nc);
      printf(" [ET %5.0f ]%s\n", et, md5_text);
    }
    sum_bits += (double)bits;
    for (int c = 0; c < 3; c++) { sum_psnr[c] += p[c]; sum_mse[c] += (double)sse[c] / (c ? nc : ny); }
    done++;
  };
  std::mutex file_mutex;                                  // reconstruction / record files: blocks are written at their own offsets
  // the app loop over one block of frames on one device: read -> device call -> per chunk of results: SSE of the output picture, the access unit (the arithmetic
  // coder), the picture hash on a pool of threads, then the output in POC order.  A single device writes as it goes; with several the access units and log rows
  // of a block are kept until every block is done.
  auto run_shard = [&](Shard &S) {
    FILE *fi = fopen(input.c_str(), "rb");
    if (!fi) { S.rc = 2; return; }
    const int sb = (int)std::min<long>(batch, S.f_hi - S.f_lo);
    // originals of one device call in page-locked memory (the upload then runs at the link's rate and does not go through a bounce buffer); label files beside them
    struct Pinned { uint8_t *p; explicit Pinned(size_t n) : p((uint8_t *)hevcdl_host_alloc(n)) {} ~Pinned() { hevcdl_host_free(p); } uint8_t *data() { return p; } } yuv_mem((size_t)src_frame_bytes * sb);
    if (!yuv_mem.data()) { fprintf(stderr, "Error: cannot allocate %zu bytes of page-locked memory for the originals\n", (size_t)src_frame_bytes * sb); S.rc = 3; fclose(fi); return; }
    std::vector<uint8_t> labels_mem(label_dir.empty() ? 0 : (size_t)ctus * 16 * sb);
    struct ChunkCtx { long f0; double et; const uint8_t *yuv; std::chrono::steady_clock::time_point t0; int nb; } cc = { 0, 0.0, nullptr, now(), 1 };
    // (with a source format the reconstruction file's frames are made on the device from the pictures in HBM: hevcdl_get_output_frames)
    const bool want_pictures = device_report ? (frec != nullptr && !use_fmt) : (frec || hash_sei || filtered), want_records = frecords != nullptr;      // what a DeviceEntropy run still fetches from HBM
    // slice_data / slice_sizes / n_sub: the packed sub-streams of the chunk's pictures (DeviceEntropy), or null: the host codes the records (hevcdl_write_access_unit)
    auto on_chunk = [&](int first, int count, const hevcdl_ctu_record *recs, const void *pictures, const hevcdl_sao_blk *sao_params, const hevcdl_frame_stats *stats,
                        const uint8_t *slice_data, const uint32_t *slice_sizes, int n_sub) -> int {
      const auto th0 = now();
      std::vector<size_t> slice_at(slice_data ? (size_t)count + 1 : 0, 0);
      for (int i = 0; slice_data && i < count; i++) { size_t n = 0; for (int k = 0; k < n_sub; k++) n += slice_sizes[(size_t)i * n_sub + k]; slice_at[(size_t)i + 1] = slice_at[(size_t)i] + n; }
      if (first == 0) cc.et = secs(cc.t0, th0) / cc.nb;                // device seconds per picture of this call (the log line's ET)
      const uint8_t *recon = (const uint8_t *)pictures;
      std::vector<PicOut> pics(count);
      std::vector<hevcdl_quality> quality(print_msssim ? count : 0);          // measured by the device call that made the pictures
      if (print_msssim) { const hevcdl_status qst = hevcdl_get_quality(S.ctx, first, count, quality.data()); if (qst != HEVCDL_OK) { fprintf(stderr, "Error: %s (status %d)\n", hevcdl_last_error(S.ctx), (int)qst); S.rc = 3; return 1; } }
      std::vector<hevcdl_picture_report_t> reports(device_report ? count : 0);      // DeviceReport: squared errors and digests of the chunk's output pictures, made by the device call
      if (device_report) { const hevcdl_status rst = hevcdl_get_picture_report(S.ctx, first, count, reports.data()); if (rst != HEVCDL_OK) { fprintf(stderr, "Error: %s (status %d)\n", hevcdl_last_error(S.ctx), (int)rst); S.rc = 3; return 1; } }
      std::vector<hevcdl_dbk_choice> choices(count);          // what every picture's slice header says about its deblocking filter (the cfg's values, or the metric's)
      { const hevcdl_status cst = hevcdl_get_dbk_choice(S.ctx, first, count, choices.data()); if (cst != HEVCDL_OK) { fprintf(stderr, "Error: %s (status %d)\n", hevcdl_last_error(S.ctx), (int)cst); S.rc = 3; return 1; } }
      std::vector<int32_t> pic_qps((size_t)count, qp);      // DeltaQpRD: the QP every picture of the chunk was coded with -- its slice_qp_delta and its log line
      if (frame_qp_keys) for (int i = 0; i < count; i++) pic_qps[(size_t)i] = seq_qps[(size_t)(cc.f0 + first + i)];      // a QP per picture: the rule's
      if (delta_qp_rd) {
        std::vector<hevcdl_qp_rd_row> qrows((size_t)count);
        const hevcdl_status qst = hevcdl_get_qp_rd(S.ctx, first, count, qrows.data(), pic_qps.data());
        if (qst != HEVCDL_OK) { fprintf(stderr, "Error: %s (status %d)\n", hevcdl_last_error(S.ctx), (int)qst); S.rc = 3; return 1; }
      }
      {
        std::atomic<int> next(0);
        auto work = [&]() {
          std::vector<uint8_t> buf(hevcdl_access_unit_bound_segments(width, height, &slices, &segments));
          hevcdl_stream_config pcfg = scfg;      // the access unit's own copy: its qp is the picture's
          for (int i = next++; i < count; i = next++) {
            if (slice_data && buf.size() < slice_at[(size_t)i + 1] - slice_at[(size_t)i] + 4096) buf.resize(2 * (slice_at[(size_t)i + 1] - slice_at[(size_t)i]) + 4096);
            PicOut &po = pics[i]; po.md5_text[0] = 0;
            for (int c = 0; c < 3; c++) po.sse[c] = stats[i].sse[c];
            bool coded_order = true;                                           // which plane order po.sse is in (the log wants the file's with YCbCrtoYCrCb, unless SNRInternalColourSpace)
            if (filtered && device_report) { for (int c = 0; c < 3; c++) po.sse[c] = reports[i].sse[c]; coded_order = false; }      // of the filtered picture, from the device
            else if (filtered && recon && use_fmt) { // the same over the window: original and output picture at the internal depth, by the library's host functions
              // (the original through the file's layout, without the explicit window; the output picture minus the padding, in the coded plane order)
              hevcdl_source_format lf = fmt; lf.output_bit_depth = bit_depth; lf.conf_win_left = lf.conf_win_right = lf.conf_win_top = lf.conf_win_bottom = 0;
              hevcdl_source_format wf = lf; wf.chroma_format = 0; wf.colour_space = 0;
              const size_t wn[3] = { (size_t)src_w * src_h, (size_t)src_w * src_h / 4, (size_t)src_w * src_h / 4 }, wtot = wn[0] + wn[1] + wn[2], ws = bit_depth > 8 ? 2 : 1;
              std::vector<uint8_t> ow(wtot * ws), rw(wtot * ws);
              if (hevcdl_load_source_host(&lf, src_w, src_h, bit_depth, cc.yuv + src_frame_bytes * (size_t)(first + i), 1, ow.data()) != HEVCDL_OK ||
                  hevcdl_store_output_host(&wf, width, height, bit_depth, recon + frame_bytes * (size_t)i, 1, rw.data()) != HEVCDL_OK) { po.st = HEVCDL_ERR_INVALID_ARG; continue; }
              size_t off = 0;
              for (int c = 0; c < 3; c++) {
                unsigned long long sse = 0;
                for (size_t k = 0; k < wn[c]; k++) { const int d = ws == 1 ? (int)ow[off + k] - (int)rw[off + k] : (int)((const uint16_t *)ow.data())[off + k] - (int)((const uint16_t *)rw.data())[off + k]; sse += (unsigned long long)(d * d); }
                po.sse[c] = sse; off += wn[c];
              }
            }
            else if (filtered && recon) { // the picture statistics follow the filtered picture: recomputed here
              const uint8_t *o = cc.yuv + frame_bytes * (size_t)(first + i), *r = recon + frame_bytes * (size_t)i;
              const size_t n[3] = { (size_t)width * height, (size_t)width * height / 4, (size_t)width * height / 4 };
              size_t off = 0;
              for (int c = 0; c < 3; c++) {
                unsigned long long sse = 0;
                if (bit_depth == 8) {
                  for (size_t k0 = 0; k0 < n[c]; k0 += 4096) { // 32-bit partial sums over short runs: the loop vectorises
                    unsigned part = 0; const size_t k1 = std::min(n[c], k0 + 4096);
                    for (size_t k = k0; k < k1; k++) { const int d = (int)o[off + k] - (int)r[off + k]; part += (unsigned)(d * d); }
                    sse += part;
                  }
                } else { const uint16_t *o16 = (const uint16_t *)o, *r16 = (const uint16_t *)r; for (size_t k = 0; k < n[c]; k++) { const int d = (int)o16[off + k] - (int)r16[off + k]; sse += (unsigned long long)(d * d); } }
                po.sse[c] = sse; off += n[c];
              }
            }
            if (file_order && coded_order) std::swap(po.sse[1], po.sse[2]);
            // the access unit: VPS+SPS+PPS+slice, written to -b; its size is the picture's bit count (TEncGOP.cpp:2420-2447)
            pcfg.qp = pic_qps[(size_t)i];
            if (slice_data) po.st = hevcdl_write_access_unit_from_slice_data_segments(&pcfg, &slices, &segments, (int)(cc.f0 + first + i), slice_data + slice_at[(size_t)i], slice_sizes + (size_t)i * n_sub, n_sub, &choices[i], buf.data(), buf.size(), &po.au_len);
            else po.st = hevcdl_write_access_unit_segments(&pcfg, &slices, &segments, (int)(cc.f0 + first + i), recs + (size_t)ctus * i, sao ? sao_params + (size_t)ctus * i : nullptr, &choices[i], buf.data(), buf.size(), &po.au_len);
            if (po.st != HEVCDL_OK) continue;
            po.bytes.assign(buf.begin(), buf.begin() + po.au_len);
            if (hash_sei) { // suffix SEI after the slice; not part of the picture's bit count (as in the reference)
              uint8_t sei[128], dg[48]; size_t sei_len = 0; int pb = 16;
              if (device_report) { memcpy(dg, reports[i].digest, sizeof dg); pb = reports[i].plane_bytes; po.st = pb > 0 && reports[i].method == hash_sei ? HEVCDL_OK : HEVCDL_ERR_INVALID_ARG; }
              else po.st = hevcdl_picture_hash(&scfg, recon + frame_bytes * (size_t)i, hash_sei, dg, &pb);
              if (po.st == HEVCDL_OK) po.st = hevcdl_write_hash_sei(hash_sei, dg, sei, sizeof sei, &sei_len);
              if (po.st != HEVCDL_OK) continue;
              po.bytes.insert(po.bytes.end(), sei, sei + sei_len);
              char *q = po.md5_text + sprintf(po.md5_text, " [%s:", hash_sei == 1 ? "MD5" : (hash_sei == 2 ? "CRC" : "Checksum"));          // TEncGOP.cpp:1160-1182
              for (int c = 0; c < 3; c++) { for (int k = 0; k < pb; k++) q += sprintf(q, "%02x", dg[pb * c + k]); *q++ = c < 2 ? ',' : ']'; }
              *q = 0;
            }
          }
        };
        const int nthreads = std::max(1, std::min(count, max_threads));
        std::vector<std::thread> pool;
        for (int t = 1; t < nthreads; t++) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
      }
      const auto tw0 = now();
      S.t_host += secs(th0, tw0);
      for (int i = 0; i < count; i++) {
        PicOut &po = pics[i];
        if (po.st != HEVCDL_OK) { fprintf(stderr, "Error: bitstream writer failed (status %d)\n", (int)po.st); S.rc = 3; return 1; }
        const long poc = cc.f0 + first + i;
        unsigned long long row[12] = { (unsigned long long)poc, (unsigned long long)po.au_len * 8, po.sse[0], po.sse[1], po.sse[2], (unsigned long long)ctus, (unsigned long long)(cc.et * 1e9), (unsigned long long)S.dev,
                                       (unsigned long long)pic_qps[(size_t)i], 0, 0, 0 };
        if (print_msssim) memcpy(row + 9, quality[i].msssim, 3 * sizeof(double));
        S.rows.insert(S.rows.end(), row, row + ROW);
        if (multi) { S.aus.push_back(std::move(po.bytes)); S.md5.push_back(po.md5_text); }
        else {
          if (fbits) fwrite(po.bytes.data(), 1, po.bytes.size(), fbits);
          log_picture(poc, pic_qps[(size_t)i], (unsigned long long)po.au_len * 8, po.sse, cc.et, po.md5_text, print_msssim ? row + 9 : nullptr);
        }
      }
      if (frec || frecords) {
        std::lock_guard<std::mutex> lock(file_mutex);
        if (frec && use_fmt) { // the window at OutputBitDepth (TVideoIOYuv.cpp:755-830)
          std::vector<uint8_t> outf(out_frame_bytes * (size_t)count);
          if ((recon ? hevcdl_store_output_host(&fmt, width, height, bit_depth, recon, count, outf.data()) : hevcdl_get_output_frames(S.ctx, first, count, outf.data())) != HEVCDL_OK) { fprintf(stderr, "Error: cannot convert the output pictures\n"); S.rc = 3; return 1; }
          if (multi) fseeko(frec, (off_t)((cc.f0 + first) * (long long)out_frame_bytes), SEEK_SET);
          fwrite(outf.data(), out_frame_bytes, count, frec);
        } else
        if (frec) { if (multi) fseeko(frec, (off_t)((cc.f0 + first) * (long long)frame_bytes), SEEK_SET); fwrite(recon, frame_bytes, count, frec); }
        if (frecords) { if (multi) fseeko(frecords, (off_t)((cc.f0 + first) * (long long)ctus * (long long)sizeof(hevcdl_ctu_record)), SEEK_SET); fwrite(recs, sizeof(hevcdl_ctu_record), (size_t)ctus * count, frecords); }
      }
      S.t_write += secs(tw0, now());
      return 0;
    };
    struct Tramp { static int call(void *u, int first, int count, const hevcdl_ctu_record *recs, const void *pics, const hevcdl_sao_blk *sp, const hevcdl_frame_stats *st)
                   { return (*(decltype(on_chunk) *)u)(first, count, recs, pics, sp, st, nullptr, nullptr, 0); }
                   static int stream(void *u, int first, int count, const uint8_t *data, const uint32_t *sizes, int n_sub, const hevcdl_frame_stats *st, const void *pics, const hevcdl_ctu_record *recs)
                   { return (*(decltype(on_chunk) *)u)(first, count, recs, pics, nullptr, st, data, sizes, n_sub); } };
    const long total = S.f_hi - S.f_lo, n_batches = (total + sb - 1) / sb;
    for (long bi = 0; bi < n_batches && S.rc == 0; bi++) {
      const long f0 = S.f_lo + bi * (long)sb; const int nb = (int)std::min<long>(sb, S.f_hi - f0);
      const auto tr0 = now();
      bool short_read = false;
      if (ts_ratio == 1) { fseeko(fi, (off_t)((frame_skip + f0) * (long long)src_frame_bytes), SEEK_SET); short_read = fread(yuv_mem.data(), src_frame_bytes, nb, fi) != (size_t)nb; }
      else for (int i = 0; i < nb && !short_read; i++) { // TemporalSubsampleRatio: picture f0 + i is source frame FrameSkip + (f0 + i) * ratio
        fseeko(fi, (off_t)((frame_skip + (f0 + i) * ts_ratio) * (long long)src_frame_bytes), SEEK_SET);
        short_read = fread(yuv_mem.data() + src_frame_bytes * (size_t)i, src_frame_bytes, 1, fi) != 1;
      }
      if (short_read) { fprintf(stderr, "Error: short read of '%s'\n", input.c_str()); S.rc = 2; break; }
      const uint8_t *lab = nullptr;
      if (!label_dir.empty()) {
        for (int i = 0; i < nb && S.rc == 0; i++) for (int a = 0; a < ctus; a++) {
          const std::string p = label_dir + "/" + std::to_string(f0 + i) + "/ctu" + std::to_string(a) + ".txt";
          std::ifstream lf(p); int v;
          for (int j = 0; j < 16; j++) { if (!(lf >> v) || v < 0 || v > 3) { fprintf(stderr, "Error: label file '%s' must hold 16 depths 0..3\n", p.c_str()); S.rc = 2; break; } labels_mem[((size_t)i * ctus + a) * 16 + j] = (uint8_t)v; }
          if (S.rc) break;
        }
        lab = labels_mem.data();
      }
      if (S.rc) break;
      const auto t0 = now();
      S.t_read += secs(tr0, t0);
      cc.f0 = f0; cc.yuv = yuv_mem.data(); cc.et = 0.0; cc.t0 = t0; cc.nb = nb;
      if (frame_qp_keys) { // this batch's slice of the sequence's QPs
        const hevcdl_status qst = hevcdl_set_frame_qps(S.ctx, seq_qps.data() + f0, nb);
        if (qst != HEVCDL_OK) { fprintf(stderr, "Error: %s (status %d)\n", hevcdl_last_error(S.ctx), (int)qst); S.rc = 3; break; }
      }
      const double host_before = S.t_host + S.t_write;
      const hevcdl_status est = device_entropy ? hevcdl_encode_pictures_stream(S.ctx, yuv_mem.data(), nb, lab, deblock ? 1 : 0, sao ? 1 : 0, want_pictures ? 1 : 0, want_records ? 1 : 0, chunk, &Tramp::stream, &on_chunk)
                                               : hevcdl_encode_pictures_chunked(S.ctx, yuv_mem.data(), nb, lab, deblock ? 1 : 0, sao ? 1 : 0, chunk, &Tramp::call, &on_chunk);
      S.t_dev += secs(t0, now()) - ((S.t_host + S.t_write) - host_before);
      if (est != HEVCDL_OK && S.rc == 0) { fprintf(stderr, "Error: %s (status %d)\n", hevcdl_last_error(S.ctx), (int)est); S.rc = 3; }
    }
    fclose(fi);
  };
  if (!multi) run_shard(shards[0]);
  else {
    std::vector<std::thread> th;
    for (int i = 1; i < n_shards; i++) th.emplace_back([&, i] { run_shard(shards[i]); });
    run_shard(shards[0]);
    for (auto &t : th) t.join();
  }
  int rc = 0;
  for (const Shard &S : shards) if (S.rc) rc = S.rc;
  if (multi && rc == 0) {
    // The per-picture rows of every device gathered with RCCL (north star: "RCCL over xGMI used only to gather per-frame rate / PSNR summaries"): one rank per
    // PHYSICAL device (ncclCommInitAll, a single process), every rank contributes the rows of its blocks padded to the largest contribution, one ncclAllGather; rank 0's
    // copy is the table the log and the summary are written from.
    std::vector<unsigned long long> table;
    std::string err, info;
    if (!gather_rows_rccl(shards.size(), [&](size_t i) { return shards[i].dev; }, [&](size_t i) -> const std::vector<unsigned long long> & { return shards[i].rows; }, ROW, table, err, &info)) {
      fprintf(stderr, "Error: gathering the per-picture rows with RCCL failed: %s\n", err.c_str()); rc = 3;
    } else {
      fprintf(stderr, "Picture rows gathered: %s\n", info.c_str());
      std::vector<const unsigned long long *> rows;
      for (size_t o = 0; o + (size_t)ROW <= table.size(); o += (size_t)ROW) if (table[o] != ~0ull) rows.push_back(&table[o]);
      std::sort(rows.begin(), rows.end(), [](const unsigned long long *a, const unsigned long long *b) { return a[0] < b[0]; });
      if ((long)rows.size() != n_frames) { fprintf(stderr, "Error: %zu rows gathered for %ld pictures\n", rows.size(), n_frames); rc = 3; }
      for (size_t r = 0; r < rows.size() && rc == 0; r++) { // POC order: blocks are contiguous, so this is the blocks one after the other
        const long poc = (long)rows[r][0];
        int si = 0; while (si + 1 < n_shards && poc >= shards[si].f_hi) si++;
        const Shard &S = shards[si];
        const size_t li = (size_t)(poc - S.f_lo);
        if (fbits) fwrite(S.aus[li].data(), 1, S.aus[li].size(), fbits);
        log_picture(poc, (int)rows[r][8], rows[r][1], rows[r] + 2, (double)rows[r][6] * 1e-9, S.md5[li].c_str(), print_msssim ? rows[r] + 9 : nullptr);
      }
    }
  }
  { double t_read = 0, t_dev = 0, t_host = 0, t_write = 0;
    for (const Shard &S : shards) { t_read = std::max(t_read, S.t_read); t_dev = std::max(t_dev, S.t_dev); t_host = std::max(t_host, S.t_host); t_write = std::max(t_write, S.t_write); }
    fprintf(stderr, "stage seconds%s: set-up (contexts, workspace) %.2f  read %.2f  device (upload + CNN + decisions + filters; its chunk copies run behind the host work) %.2f  host (entropy coding, hashes, %d threads) %.2f  write %.2f  whole run %.2f\n",
            multi ? " (slowest device)" : "", t_setup, t_read, t_dev, max_threads, t_host, t_write, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_main0).count()); }
  if (rc == 0 && done > 0) { // TEncAnalyze::printOut, 4:2:0 layout
    const double mse_yuv = (4 * sum_mse[0] + sum_mse[1] + sum_mse[2]) / done / 6.0;
    printf("\n\nSUMMARY --------------------------------------------------------\n");
    const double psnr_yuv = mse_yuv == 0 ? 999.99 : 10.0 * log10((double)(255 << (bit_depth - 8)) * (double)(255 << (bit_depth - 8)) / mse_yuv);
    if (!print_msssim && !print_seq_mse) {
      printf("\tTotal Frames |   Bitrate     Y-PSNR    U-PSNR    V-PSNR    YUV-PSNR  \n");
      printf("\t %8ld    %c %12.4lf  %8.4lf  %8.4lf  %8.4lf  %8.4lf  \n", done, 'a', sum_bits * (fps / (double)ts_ratio / 1000.0 / done), sum_psnr[0] / done, sum_psnr[1] / done, sum_psnr[2] / done, psnr_yuv);
    } else { // the extra columns of TEncAnalyze.h:315-388
      printf("\tTotal Frames |   Bitrate     Y-PSNR    U-PSNR    V-PSNR    YUV-PSNR  ");
      if (print_msssim) printf("  Y-MS-SSIM    U-MS-SSIM    V-MS-SSIM  ");
      printf(print_seq_mse ? "  Y-MSE     U-MSE     V-MSE     YUV-MSE  \n" : "\n");
      printf("\t %8ld    %c %12.4lf  %8.4lf  %8.4lf  %8.4lf  %8.4lf  ", done, 'a', sum_bits * (fps / (double)ts_ratio / 1000.0 / done), sum_psnr[0] / done, sum_psnr[1] / done, sum_psnr[2] / done, psnr_yuv);
      if (print_msssim) printf("   %8.6lf     %8.6lf     %8.6lf  ", sum_msssim[0] / (double)done, sum_msssim[1] / (double)done, sum_msssim[2] / (double)done);
      if (print_seq_mse) { // MSEyuv as calculateCombinedValues adds it up (TEncAnalyze.h:180-194)
        double acc = 0; acc += 4 * (sum_mse[0] / (double)done); acc += 1 * (sum_mse[1] / (double)done); acc += 1 * (sum_mse[2] / (double)done);
        printf(" %8.4lf  %8.4lf  %8.4lf  %8.4lf  \n", sum_mse[0] / (double)done, sum_mse[1] / (double)done, sum_mse[2] / (double)done, acc / 6.0);
      } else printf("\n");
    }
  }
  if (frec) fclose(frec);
  if (frecords) fclose(frecords);
  if (fbits) fclose(fbits);
  for (Shard &S : shards) hevcdl_destroy(S.ctx);
  return rc;
}
