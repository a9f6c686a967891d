// Optional timing of the denoiser's GEMM launches with hipEvents on the launch stream (ditree_profile / ditree_profile_read).
#pragma once
#include <vector>

#include "denoise.h"

struct DenoiseProfiler {
  bool on = false;
  int mode = 0;                  // 1: every MFMA launch, 2: only runs of the dominant (halo) kernel, one event pair per run
  int ufmt = 0;                  // format of the U-Net GEMMs of the current workspace: what mode 2 calls dominant
  // per kernel kind: 0 = conv3_halo_kernel, 1 = conv_gemm_kernel, 2 = conv_gemm_kernel (implicit Conv2d)
  double ms_done[3] = {0, 0, 0};
  int64_t launches_done[3] = {0, 0, 0};
  double flops_done[3] = {0, 0, 0};

  ~DenoiseProfiler() {
    for (auto e : ev) hipEventDestroy(e);
  }
  // ditree_profile: account what is pending, switch the mode, start from zero when switching on
  void set(int enable) {
    collect();
    on = enable != 0;
    mode = enable;
    if (enable) for (int k = 0; k < 3; ++k) { ms_done[k] = 0.0; launches_done[k] = 0; flops_done[k] = 0.0; }
  }
  // Profiling brackets every GEMM launch with events on its stream.  Back-to-back GEMM launches on
  // one stream share an event (the end of one is the start of the next), which halves the marker
  // packets; `chain` is broken by note_other() whenever another kernel is enqueued in between.
  void note_other() { close_run(); chain = false; }          // call BEFORE enqueueing the other kernel
  void launch(const ConvGemmParams& p, int fmt, hipStream_t s) {
    if (!on) { launch_conv_gemm(p, fmt, s); return; }
    if (used + 2 > ev.size()) {
      const size_t old = ev.size();
      ev.resize(old + 4096);
      for (size_t i = old; i < ev.size(); ++i) hipEventCreate(&ev[i]);
    }
    const double fl = 2.0 * (double)p.M * (double)p.N * (double)p.taps * (double)p.Cin;
    if (mode == 2) {
      // dominant kernel only: one (start, end) pair around each run of back-to-back halo launches, so the timed
      // region carries ~20 marker packets per denoiser call instead of ~120
      const int dom = fmt_st(ufmt) == ST_F32 ? 1 : 0;        // f32 instantiation: everything runs on conv_gemm_kernel
      if (conv_gemm_kind(p, fmt) != dom || fmt != ufmt) { close_run(); launch_conv_gemm(p, fmt, s); return; }
      if (run_open && last_stream == s) {
        launch_conv_gemm(p, fmt, s);
        pairs.back().flops += fl;
        pairs.back().launches += 1;
        return;
      }
      close_run();
      const size_t st = used++;
      run_end = used++;
      hipEventRecord(ev[st], s);
      launch_conv_gemm(p, fmt, s);
      pairs.push_back(Rec{st, run_end, dom, fl, 1});
      run_open = true;
      last_stream = s;
      return;
    }
    size_t start;
    if (chain && last_stream == s && used > 0) {
      start = used - 1;
    } else {
      start = used++;
      hipEventRecord(ev[start], s);
    }
    launch_conv_gemm(p, fmt, s);
    const size_t end = used++;
    hipEventRecord(ev[end], s);
    pairs.push_back(Rec{start, end, conv_gemm_kind(p, fmt), fl, 1});
    chain = true;
    last_stream = s;
  }
  void collect() {
    close_run();
    if (used == 0) return;
    hipDeviceSynchronize();                                  // events live on several streams
    for (auto& pr : pairs) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[pr.a], ev[pr.b]) == hipSuccess) ms_done[pr.kind] += ms;
      launches_done[pr.kind] += pr.launches;
      flops_done[pr.kind] += pr.flops;
    }
    pairs.clear();
    used = 0;
    chain = false;
  }

 private:
  struct Rec { size_t a, b; int kind; double flops; int launches; };
  std::vector<hipEvent_t> ev;
  size_t used = 0;
  std::vector<Rec> pairs;        // (start event, end event, kind, flops) per launch or run
  bool run_open = false;         // mode 2: a run of back-to-back halo launches whose end event is still to be recorded
  size_t run_end = 0;
  hipStream_t last_stream = nullptr;
  bool chain = false;
  void close_run() {
    if (run_open) { hipEventRecord(ev[run_end], last_stream); run_open = false; }
  }
};
