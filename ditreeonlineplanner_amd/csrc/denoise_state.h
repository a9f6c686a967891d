// The denoiser's state: loaded parameters, the workspace of one reservation, the launch plan and its run state.
// denoise_plan.hip builds the workspace and the plan, denoise_host.hip loads the weights and runs the plan.
#pragma once
#include <functional>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "denoise.h"
#include "denoise_prof.h"
#include "ditree_internal.h"

struct HostParam {
  std::vector<int64_t> dims;
  const float* data = nullptr;
  int64_t n = 0;
};

struct Act {             // channels-last activation view
  void* p = nullptr;
  int L = 0, C = 0;      // positions per sample, channels of this view
  int ld = 0, coff = 0;  // row stride (elements), channel offset of the view
  bool padded = true;    // rows per sample = L + 2 (one zero row each side)
  long long plane = 0;   // split formats: bytes from the hi plane to the lo plane (same layout)
  int fmt = 0;           // numeric format of the buffer (denoise.h)
  int Lp() const { return padded ? L + 2 : L; }
};

struct Packed {          // a GEMM weight in the MFMA layout
  void* p = nullptr;
  long long plane = 0;   // split formats: bytes from an element's hi half to its lo half
  int row_bytes = 0;     // split formats: bytes per weight row, and between the 32-channel chunks of a row
  int chunk_step = 0;    //   (ConvGemmParams::w_row / w_step: chunk-interleaved or planar)
  float scale = 1.0f;    // f16: the stored values are w / scale (scale a power of two)
};

struct TapList {         // live (kh, kw) taps of a Conv2d on a small map: the first 12 of n (ConvGemmParams::c2_kh)
  int n;
  signed char kh[12], kw[12];
};

struct DenoiserState {
  using Op = std::function<void(int, int, hipStream_t)>;     // (B, Bp, stream): the samples of a call, and padded to `bgran`
  ditree_ctx* ctx = nullptr;
  std::vector<float> blob;
  std::map<std::string, HostParam> params;
  // architecture (derived from the parameter shapes)
  int D = 2, P = 64, E = 400, G = 7, cond_dim = 663, lm = 20;
  int enc_kind = ENC_RESNET;   // "#encoder <name> <E>" of the manifest (none: resnet)
  int enc_E = -1;              // the width that line declares (-1: none)
  int enc_k = 0;               // max: cells per side
  int dims[3] = {512, 1024, 2048};
  bool loaded = false;
  // DDPM loop of the NEXT denoise call (set by denoise_run_ddpm around denoise_core): coef (K, 5) = sb, sa, c0, c1, sigma per step
  const float* ddpm_coef = nullptr;
  const float* ddpm_z = nullptr;           // [dev] step noise, row r / step k at r * z_row + k * z_step
  long long ddpm_z_row = 0, ddpm_z_step = 0;
  int ddpm_row0 = 0;                       // first row of the current sub-batch (dense calls)
  // workspace
  int prec = -1, Bmax = 0;     // prec: the DITREE_PREC_* the workspace was built for; Bmax: samples the WORKSPACE holds
  int Buser = 0;               // samples the caller reserved for: calls up to this size are served in sub-batches of <= Bmax
  int bgran = 16;              // batch rows are padded to a multiple of this
  int ufmt = 0, efmt = 0;      // formats (denoise.h) of the U-Net activations / GEMMs and of the encoder
  bool split_planar = false;   // DITREE_SPLIT_PLANAR=1 (read by build): split weights as two planes instead of chunk-interleaved
  std::vector<void*> allocs;
  std::map<std::string, Act> named;
  std::map<std::string, Packed> dev_w;      // packed GEMM weights by name
  std::map<std::string, float*> dev_f;      // f32 vectors (bias, gamma, beta, small matrices)
  std::vector<Op> unet_ops, enc_ops;
  Op film_op;
  float* x_cur = nullptr;        // (Bmax, P, D) f32
  float* temb = nullptr;         // (256,) f32
  float temb_t = -1.0f;          // timestep the cached embedding was computed for (< 0: none)
  float* map_emb = nullptr;      // (Brows, E_ld) f32
  int E_ld = 400;                // row stride of map_emb (E, or E padded to 256 for the split encoder's fc tiles)
  float* film = nullptr;         // (Brows, film_cols) f32
  void* condA = nullptr;         // (Brows, condK) [x planes]
  long long cond_plane = 0;
  int condK = 0, film_cols = 0;
  Act final_h;                   // input of the final 1x1 projection
  const float* lm_ptr = nullptr; // caller's scaled local map of the current call
  // f16 range guard (denoise_device.h sat_*): one device flag word per layer that stores f16 activations; a kernel ORs 1
  // into its layer's word when it is handed a value beyond +-65504.  Sticky until ditree_denoise_status reads and clears.
  static constexpr int SAT_SLOTS = 256;
  int* sat_flags = nullptr;
  int *sat_cond = nullptr, *sat_sample = nullptr;      // slots of the two input-preparation kernels
  std::vector<std::string> sat_names;
  DenoiseProfiler prof;
  // Latency mode (DITREE_DENOISE_SPLITK=1, read per call; opt-in): below ~ 256 candidates a layer is a handful of 256 x 256 tiles
  // and the K loop of ONE tile (up to 384 K-steps) is the layer's latency while most CUs idle.  The 3-tap convs of the split
  // formats then run `splitk` work-groups per tile (each a contiguous share of the channel chunks), the last one adds the partial
  // accumulators in split order and runs the fused epilogue.  Deterministic, but NOT bit-identical to the one-pass sum: with
  // the mode on, a sample's result depends on whether its batch was small enough to split -- which is why it is opt-in and why
  // a sharded planner must switch it by its GLOBAL batch.
  float* sk_ws = nullptr;
  int* sk_cnt = nullptr;
  static constexpr int SK_MAX_SLABS = 512;                   // 512 x 256 KB = 128 MB of partial tiles

  int es() const { return fmt_es(ufmt); }                   // element bytes of a U-Net activation plane
  int planes() const { return fmt_split(ufmt) ? 2 : 1; }
  int Brows() const { return (Bmax + 255) / 256 * 256; }    // matrix GEMMs (FiLM, the split encoder's fc) run on whole 256-row tiles
  const HostParam& P_(const std::string& name) const {
    auto it = params.find(name);
    if (it == params.end()) throw std::runtime_error("missing parameter " + name);
    return it->second;
  }
  bool has(const std::string& name) const { return params.count(name) != 0; }

  // ---- denoise_plan.hip
  void build(int prec_, int Bmax_);              // workspace and plan of one reservation (frees the previous one)
  void free_workspace();
  void run_gemm(const ConvGemmParams& p_in, int fmt, hipStream_t s);

 private:
  int* sat_slot(const std::string& layer, int fmt);
  int pick_splitk(const ConvGemmParams& p, int fmt);
  void* dalloc(size_t bytes, bool zero = true);
  float* upload_f32(const std::string& key, const float* src, int64_t n);
  float* vec(const std::string& name);
  template <class F>
  Packed pack(const std::string& key, int fmt, int N, int T, int Cin_pad, F get);
  Act make_act(const std::string& name, int L, int C, bool padded, int fmt, int rows);
  Act make_act(const std::string& name, int L, int C, bool padded = true);       // ... of Bmax samples in the U-Net's format
  const char* aptr(const Act& a) const { return (const char*)a.p + (size_t)a.coff * es(); }
  ConvGemmParams gemm_params(const Act& in, const Act& out, const Packed& wp, int taps, int Cin, int Cout, int in_stride, int in_off,
                             int out_stride, int out_off, int L, const float* bias, int* sat);
  ConvGemmParams gemm_params(const Act& in, const Act& out, const Packed& wp, int taps, int Cin, int Cout, int in_stride, int in_off,
                             int out_stride, int out_off, int L, const std::string& wname);
  void set_epilogue(ConvGemmParams& p, int mode, const std::string& gn, int film_off, const Act* res);
  void run_rows(ConvGemmParams p, int rows, bool whole_tiles, int fmt, hipStream_t s);
  // U-Net op builders: each appends to unet_ops
  void push_gemm(const ConvGemmParams& p_in);
  void emit_block(const ConvGemmParams& p, const Act& out);
  void add_conv3(const std::string& wname, const Act& in, const Act& out, int mode, const std::string& gn, int film_off,
                 const Act* res);
  void add_conv1(const std::string& wname, const Act& in, const Act& out);
  void add_down(const std::string& wname, const Act& in, const Act& out);
  void add_up(const std::string& wname, const Act& in, const Act& out);
  void add_crb(const std::string& pre, const Act& in, const Act& out, int& film_cursor, const std::string& tag);
  void build_film();
  void build_unet();
  void build_encoder_small();
  void build_encoder_resnet();
  void validate_plan();
};
