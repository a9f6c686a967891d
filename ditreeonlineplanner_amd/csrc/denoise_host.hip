// Host side of the denoiser: weight loading, the sampler loops over the plan of denoise_plan.hip, the C ABI.
//
// Reference structure reproduced:
//   policies/fm_policy.py:183-203  flow steps x <- x + v*dt[k]; a = x*sigma + mu
//   policies/fm_policy.py:164-182  the DDPM branch
#include <algorithm>
#include <cstring>
#include <sstream>

#include "denoise_state.h"

static int parse_manifest(DenoiserState* st, const char* manifest, int64_t n_floats) {
  std::istringstream in(manifest);
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    if (line.rfind("#config", 0) == 0) {          // "#config pred_horizon 64 local_map_size 20": what the shapes do not tell
      std::istringstream cs(line.substr(7));
      std::string key;
      int val;
      while (cs >> key >> val) {
        if (key == "pred_horizon") st->P = val;
        else if (key == "local_map_size") st->lm = val;
      }
      continue;
    }
    if (line.rfind("#encoder", 0) == 0) {         // "#encoder cnn 576": the local-map encoder and its embedding width
      std::istringstream cs(line.substr(8));
      std::string kind;
      if (!(cs >> kind)) return -1;
      st->enc_kind = -1;
      for (int k = ENC_RESNET; k <= ENC_CNN; ++k)
        if (kind == small_encoder_name(k)) st->enc_kind = k;
      if (st->enc_kind < 0) return -3;
      int e;
      if (cs >> e) st->enc_E = e;
      continue;
    }
    if (line.rfind("#checksum", 0) == 0) {        // "#checksum <s1 hex> <s2 hex>": Fletcher-style sums over the blob's 32-bit words
      std::istringstream cs(line.substr(9));
      std::string a, b;
      if (!(cs >> a >> b)) return -1;
      const uint32_t* w = (const uint32_t*)st->blob.data();
      uint64_t s1 = 0, s2 = 0;
      for (int64_t i = 0; i < n_floats; ++i) { s1 += w[i]; s2 += s1; }
      if (s1 != std::stoull(a, nullptr, 16) || s2 != std::stoull(b, nullptr, 16)) return -2;
      continue;
    }
    if (line[0] == '#') continue;
    std::istringstream ls(line);
    std::string name;
    int64_t off, n;
    int nd;
    if (!(ls >> name >> off >> n >> nd)) return -1;
    HostParam hp;
    int64_t prod = 1;
    for (int i = 0; i < nd; ++i) {
      int64_t d;
      if (!(ls >> d)) return -1;
      hp.dims.push_back(d);
      prod *= d;
    }
    if (prod != n || off < 0 || off + n > n_floats) return -1;
    hp.data = st->blob.data() + off;
    hp.n = n;
    st->params[name] = hp;
  }
  return 0;
}

static int denoise_core(ditree_ctx* ctx, const float* noise, int64_t noise_stride, const int32_t* noise_idx,
                        const float* local_map, const float* cond, int B, int K, const float* t0, const float* dt,
                        const double* act_norm, double* actions, float* x_out, hipStream_t s, float t_scale, int raw,
                        int reuse_encoder);

static int denoise_core_one(ditree_ctx* ctx, const float* noise, int64_t noise_stride, const int32_t* noise_idx,
                            const float* local_map, const float* cond, int B, int K, const float* t0, const float* dt,
                            const double* act_norm, double* actions, float* x_out, hipStream_t s, float t_scale, int raw,
                            int reuse_encoder);

// The DDPM branch of the sampler (policies/fm_policy.py:164-182) as K steps inside the library: timesteps[k] is what the
// sinusoidal embedding sees (the scheduler's integer k, NOT scaled by 20), coef (K, 5) the step's sb, sa, c0, c1, sigma,
// z [dev] the standard-normal step noise (row r, step k at r * z_row + k * z_step; rows by noise_idx like the start noise).
int denoise_run_ddpm(ditree_ctx* ctx, const float* noise, int64_t noise_stride, const int32_t* noise_idx, const float* local_map,
                     const float* cond, int B, int K, const float* timesteps, const float* coef, const float* z, int64_t z_row,
                     int64_t z_step, const double* act_norm, double* actions, float* x_out, hipStream_t s) {
  DenoiserState* st = ctx->dn;
  if (!st || !st->loaded) return set_err(ctx, DITREE_E_STATE, "denoise: weights not loaded");
  if (!coef || !timesteps || K < 1) return set_err(ctx, DITREE_E_ARG, "denoise_ddpm: schedule missing");
  std::vector<float> ones((size_t)K, 1.0f);
  st->ddpm_coef = coef; st->ddpm_z = z; st->ddpm_z_row = z_row; st->ddpm_z_step = z_step; st->ddpm_row0 = 0;
  const int rc = denoise_core(ctx, noise, noise_stride, noise_idx, local_map, cond, B, K, timesteps, ones.data(), act_norm, actions,
                              x_out, s, 1.0f, 0, 0);
  st->ddpm_coef = nullptr; st->ddpm_z = nullptr;
  return rc;
}

// Candidates per full wave of 256-row x 256-channel tiles over the chip's 256 CUs at the U-Net levels (all levels have the same
// number of tiles: rows halve as channels double): 256 * 65536 / (P * down_dims[0]) -- 512 for the car network (P 64, 512
// channels), 2048 for the ant network (P 16).  What early-exit rounds pack their denoiser calls to.
int denoise_wave_quantum(ditree_ctx* ctx) {
  DenoiserState* st = ctx->dn;
  if (!st || !st->loaded) return 512;
  const long long q = 256ll * 65536ll / ((long long)st->P * st->dims[0]);
  return (int)std::max(64ll, std::min(q, 65536ll));
}

int denoise_run(ditree_ctx* ctx, const float* noise, int64_t noise_stride, const int32_t* noise_idx, const float* local_map,
                const float* cond, int B, int K, const float* t0, const float* dt, const double* act_norm, double* actions,
                float* x_out, hipStream_t s) {
  return denoise_core(ctx, noise, noise_stride, noise_idx, local_map, cond, B, K, t0, dt, act_norm, actions, x_out, s,
                      20.0f /* pos_emb_scale, fm_policy.py:187 */, 0, 0);
}

// A call of up to the reserved batch: rows are independent, so it runs as sub-batches of at most the workspace size (every
// pointer advances by the rows done; a compacted round's noise index list advances with them).
static int denoise_core(ditree_ctx* ctx, const float* noise, int64_t noise_stride, const int32_t* noise_idx,
                        const float* local_map, const float* cond, int B, int K, const float* t0, const float* dt,
                        const double* act_norm, double* actions, float* x_out, hipStream_t s, float t_scale, int raw,
                        int reuse_encoder) {
  DenoiserState* st = ctx->dn;
  if (!st || !st->loaded) return set_err(ctx, DITREE_E_STATE, "denoise: weights not loaded");
  if (st->prec < 0) return set_err(ctx, DITREE_E_STATE, "denoise: call ditree_denoise_reserve first");
  if (B <= 0 || B > st->Buser) return set_err(ctx, DITREE_E_ARG, "denoise: batch exceeds the reserved workspace");
  if (B <= st->Bmax)
    return denoise_core_one(ctx, noise, noise_stride, noise_idx, local_map, cond, B, K, t0, dt, act_norm, actions, x_out, s,
                            t_scale, raw, reuse_encoder);
  if (!noise || !local_map || !cond) return set_err(ctx, DITREE_E_ARG, "denoise: bad argument");
  const size_t PD = (size_t)st->P * st->D, LM = (size_t)st->lm * st->lm;
  const int row0 = st->ddpm_row0;
  for (int b0 = 0; b0 < B; b0 += st->Bmax) {
    const int bn = std::min(st->Bmax, B - b0);
    st->ddpm_row0 = row0 + (noise_idx ? 0 : b0);
    // (the map embedding of a previous call covers one sub-batch only: larger calls recompute it)
    const int rc = denoise_core_one(ctx, noise_idx ? noise : noise + (size_t)b0 * noise_stride, noise_stride,
                                    noise_idx ? noise_idx + b0 : nullptr, local_map + (size_t)b0 * LM, cond + (size_t)b0 * st->G, bn,
                                    K, t0, dt, act_norm, actions ? actions + (size_t)b0 * PD : nullptr,
                                    x_out ? x_out + (size_t)b0 * PD : nullptr, s, t_scale, raw, 0);
    if (rc) { st->ddpm_row0 = row0; return rc; }
  }
  st->ddpm_row0 = row0;
  return DITREE_OK;
}

// t_scale: factor on t0[k] before the sinusoidal embedding (20 for the flow sampler, 1 for a raw evaluation);
// raw: the last projection writes the network output instead of the Euler update; reuse_encoder: keep the map
// embedding of the previous call (same local maps: the steps of a DDPM loop).
static int denoise_core_one(ditree_ctx* ctx, const float* noise, int64_t noise_stride, const int32_t* noise_idx,
                            const float* local_map, const float* cond, int B, int K, const float* t0, const float* dt,
                            const double* act_norm, double* actions, float* x_out, hipStream_t s, float t_scale, int raw,
                            int reuse_encoder) {
  DenoiserState* st = ctx->dn;
  if (B <= 0 || B > st->Bmax) return set_err(ctx, DITREE_E_ARG, "denoise: batch exceeds the workspace");
  if (!noise || !local_map || !cond || !t0 || !dt || !act_norm || K <= 0 || (!actions && !x_out))
    return set_err(ctx, DITREE_E_ARG, "denoise: bad argument");
  const int Bp = (B + st->bgran - 1) / st->bgran * st->bgran;
  const int uf = st->ufmt;
  {
    const size_t row = (size_t)st->P * st->D * 4;         // one candidate's (P, D) f32 noise
    if (noise_stride < (int64_t)st->P * st->D) return set_err(ctx, DITREE_E_ARG, "denoise: noise stride");
    if (noise_idx)                                       // compacted round: row r takes candidate noise_idx[r]'s noise
      launch_gather_rows_f32(noise, noise_stride, noise_idx, st->x_cur, st->P * st->D, B, s);
    else
      HIP_TRY(ctx, hipMemcpy2DAsync(st->x_cur, row, noise, (size_t)noise_stride * 4, row, (size_t)B,
                                    hipMemcpyDeviceToDevice, s));
  }
  st->lm_ptr = local_map;
  try {
  if (!reuse_encoder)
    for (auto& op : st->enc_ops) op(B, Bp, s);
  for (int k = 0; k < K; ++k) {
    const float t = t0[k] * t_scale;
    if (t != st->temb_t) {                                              // batch-invariant: K = 1 computes it once
      launch_time_embed(t, st->dev_f["unet.diffusion_step_encoder.1.weight"], st->dev_f["unet.diffusion_step_encoder.1.bias"],
                        st->dev_f["unet.diffusion_step_encoder.3.weight"], st->dev_f["unet.diffusion_step_encoder.3.bias"],
                        st->temb, s);
      st->temb_t = K == 1 ? t : -1.0f;                                  // several steps share one buffer: recompute
    }
    st->prof.note_other();
    launch_prep_cond(st->temb, st->map_emb, st->E, st->E_ld, cond, st->G, st->condA, B, Bp, st->condK, uf, st->cond_plane, s,
                     st->sat_cond);
    st->film_op(B, Bp, s);
    st->prof.note_other();
    launch_prep_sample(st->x_cur, st->named["a0"].p, B, Bp, st->P, st->D, uf, st->named["a0"].plane, s,
                       st->sat_sample);
    for (auto& op : st->unet_ops) op(B, Bp, s);
    const bool last = (k == K - 1);
    st->prof.note_other();
    FlowStep fs{};
    fs.mode = raw ? 1 : 0;
    fs.dt = dt[k];
    if (st->ddpm_coef) {
      const float* c = st->ddpm_coef + 5 * k;
      fs.mode = 2; fs.sb = c[0]; fs.sa = c[1]; fs.c0 = c[2]; fs.c1 = c[3]; fs.sigma = c[4];
      fs.z = st->ddpm_z ? st->ddpm_z + (long long)k * st->ddpm_z_step : nullptr;
      fs.z_row = st->ddpm_z_row; fs.z_idx = noise_idx; fs.z_row0 = st->ddpm_row0;
      if (fs.sigma != 0.0f && !fs.z) return set_err(ctx, DITREE_E_ARG, "denoise: a DDPM step with sigma > 0 needs step noise");
    }
    launch_final_proj_flow(st->final_h.p, st->final_h.C, st->final_h.Lp(), st->final_h.plane, st->dev_f["unet.final_conv.1.weight"],
                           st->dev_f["unet.final_conv.1.bias"], st->D, st->x_cur, fs, act_norm,
                           (last && actions) ? actions : nullptr, B, st->P, uf, s);
  }
  } catch (const std::exception& e) {
    return set_err(ctx, DITREE_E_ARG, std::string("denoise: ") + e.what());
  }
  if (x_out) HIP_TRY(ctx, hipMemcpyAsync(x_out, st->x_cur, (size_t)B * st->P * st->D * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

void denoise_destroy(ditree_ctx* ctx) {
  if (ctx->dn) {
    ctx->dn->free_workspace();
    delete ctx->dn;                    // (the profiler's events go with it)
    ctx->dn = nullptr;
  }
}

extern "C" {

int32_t ditree_load_weights(ditree_ctx* ctx, const float* blob, int64_t n_floats, const char* manifest, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!blob || !manifest || n_floats <= 0) return set_err(ctx, DITREE_E_ARG, "load_weights: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  denoise_destroy(ctx);
  DenoiserState* st = new (std::nothrow) DenoiserState();
  if (!st) return set_err(ctx, DITREE_E_NOMEM, "load_weights: out of memory");
  st->ctx = ctx;
  try {
    st->blob.assign(blob, blob + n_floats);
    const int prc = parse_manifest(st, manifest, n_floats);
    if (prc == -2) throw std::runtime_error("weight blob does not match the manifest checksum");
    if (prc == -3) throw std::runtime_error("unknown encoder in the manifest (identity, mlp, max, grid, cnn or resnet)");
    if (prc != 0) throw std::runtime_error("malformed manifest");
    const HostParam& w0 = st->P_("unet.down_modules.0.0.blocks.0.block.0.weight");
    st->D = (int)w0.dims[1];
    for (int i = 0; i < 3; ++i)
      st->dims[i] = (int)st->P_("unet.down_modules." + std::to_string(i) + ".0.blocks.0.block.0.weight").dims[0];
    if (st->has("unet.down_modules.3.0.blocks.0.block.0.weight")) throw std::runtime_error("only 3 U-Net levels supported");
    st->cond_dim = (int)st->P_("unet.down_modules.0.0.cond_encoder.1.weight").dims[1];
    if (st->lm != 20 && st->lm != 16) throw std::runtime_error("local_map_size must be 20 (car) or 16 (ant)");
    if (st->enc_kind == ENC_RESNET) {
      st->E = (int)st->P_("encoder.resnet18.fc.weight").dims[0];
      if (st->enc_E >= 0 && st->enc_E != st->E) throw std::runtime_error("the manifest's encoder width differs from encoder.resnet18.fc");
    } else {
      // the width follows from the kind and the map size; 'max' pools to k x k cells and takes k from the declared width
      const std::string kn = small_encoder_name(st->enc_kind);
      if (st->enc_E < 1) throw std::runtime_error("the manifest's #encoder line must carry the embedding width");
      st->enc_k = 0;
      if (st->enc_kind == ENC_MAX) {
        int k = 1;
        while ((k + 1) * (k + 1) <= st->enc_E) ++k;
        if (k * k != st->enc_E) throw std::runtime_error("encoder 'max': the embedding width must be a perfect square, got " + std::to_string(st->enc_E));
        st->enc_k = k;
      }
      st->E = small_encoder_width(st->enc_kind, st->lm, st->enc_k);
      if (st->E != st->enc_E)
        throw std::runtime_error("encoder '" + kn + "' produces " + std::to_string(st->E) + " columns at local_map_size " +
                                 std::to_string(st->lm) + ", the manifest declares " + std::to_string(st->enc_E));
    }
    st->G = st->cond_dim - 256 - st->E;
    if (st->G < 0 && st->enc_kind != ENC_RESNET)
      throw std::runtime_error("the U-Net's cond_dim " + std::to_string(st->cond_dim) + " is narrower than 256 + the encoder's " +
                               std::to_string(st->E) + " columns");
    if (st->G < 0 || (st->D != 2 && st->D != 8)) throw std::runtime_error("unsupported dimensions (action_dim 2 or 8)");
    if (st->P_("unet.diffusion_step_encoder.1.weight").dims[1] != 256) throw std::runtime_error("diffusion_step_embed_dim must be 256");
    for (int i = 0; i < 3; ++i)
      if (st->dims[i] % 64 != 0 || st->dims[i] > 4096) throw std::runtime_error("down_dims must be multiples of 64, <= 4096");
  } catch (const std::exception& e) {
    delete st;
    return set_err(ctx, DITREE_E_ARG, std::string("load_weights: ") + e.what());
  }
  st->loaded = true;
  ctx->dn = st;
  (void)stream;
  return DITREE_OK;
}

int32_t ditree_denoise_reserve(ditree_ctx* ctx, int32_t max_batch, int32_t precision) {
  if (!ctx) return DITREE_E_ARG;
  DenoiserState* st = ctx->dn;
  if (!st || !st->loaded) return set_err(ctx, DITREE_E_STATE, "denoise_reserve: weights not loaded");
  if (max_batch <= 0 || precision < DITREE_PREC_BF16 || precision > DITREE_PREC_F16)
    return set_err(ctx, DITREE_E_ARG, "denoise_reserve: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (st->prec == precision && st->Buser >= max_batch) return DITREE_OK;
  try {
    HIP_TRY(ctx, hipDeviceSynchronize());
    st->build(precision, max_batch);
  } catch (const std::exception& e) {
    st->free_workspace();
    return set_err(ctx, DITREE_E_NOMEM, std::string("denoise_reserve: ") + e.what());
  }
  return DITREE_OK;
}

int32_t ditree_denoise(ditree_ctx* ctx, const float* noise, const float* local_map, const float* cond, int32_t B,
                       int32_t K, const float* t0, const float* dt, const double* act_norm, double* actions,
                       float* x_out, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->dn) return set_err(ctx, DITREE_E_STATE, "denoise: weights not loaded");
  return denoise_run(ctx, noise, (int64_t)ctx->dn->P * ctx->dn->D, nullptr, local_map, cond, B, K, t0, dt, act_norm, actions, x_out,
                     (hipStream_t)stream);
}

int32_t ditree_denoise_ddpm(ditree_ctx* ctx, const float* noise, const float* step_noise, const float* local_map, const float* cond,
                            int32_t B, int32_t K, const float* timesteps, const float* coef, const double* act_norm,
                            double* actions, float* x_out, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->dn) return set_err(ctx, DITREE_E_STATE, "denoise_ddpm: weights not loaded");
  if (B == 0) return DITREE_OK;
  const int64_t PD = (int64_t)ctx->dn->P * ctx->dn->D;
  return denoise_run_ddpm(ctx, noise, PD, nullptr, local_map, cond, B, K, timesteps, coef, step_noise, (int64_t)K * PD, PD, act_norm,
                          actions, x_out, (hipStream_t)stream);
}

int32_t ditree_denoise_eval(ditree_ctx* ctx, const float* sample, const float* local_map, const float* cond, int32_t B,
                            float timestep, int32_t reuse_encoder, float* out, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->dn) return set_err(ctx, DITREE_E_STATE, "denoise_eval: weights not loaded");
  if (!out) return set_err(ctx, DITREE_E_ARG, "denoise_eval: bad argument");
  const float one = 1.0f;
  double unit[16];
  for (int d = 0; d < 8; ++d) { unit[d] = 0.0; unit[8 + d] = 1.0; }
  for (int d = 0; d < ctx->dn->D && d < 8; ++d) { unit[d] = 0.0; unit[ctx->dn->D + d] = 1.0; }
  return denoise_core(ctx, sample, (int64_t)ctx->dn->P * ctx->dn->D, nullptr, local_map, cond, B, 1, &timestep, &one, unit,
                      nullptr, out, (hipStream_t)stream, 1.0f, 1, reuse_encoder);
}

int32_t ditree_denoise_dims(ditree_ctx* ctx, int32_t* dims5) {
  if (!ctx) return DITREE_E_ARG;
  DenoiserState* st = ctx->dn;
  if (!st || !st->loaded || !dims5) return set_err(ctx, DITREE_E_STATE, "denoise_dims: weights not loaded");
  dims5[0] = st->P; dims5[1] = st->D; dims5[2] = st->lm; dims5[3] = st->G; dims5[4] = st->E;
  return DITREE_OK;
}

int32_t ditree_denoise_status(ditree_ctx* ctx, int32_t* n_saturated, char* names, int64_t names_cap, int32_t clear,
                              void* stream) {
  if (!ctx) return DITREE_E_ARG;
  DenoiserState* st = ctx->dn;
  if (!n_saturated || (names_cap > 0 && !names)) return set_err(ctx, DITREE_E_ARG, "denoise_status: bad argument");
  *n_saturated = 0;
  if (names_cap > 0) names[0] = '\0';
  if (!st || st->prec < 0 || st->sat_flags == nullptr || st->sat_names.empty()) return DITREE_OK;   // nothing can saturate
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> host(st->sat_names.size());
  HIP_TRY(ctx, hipMemcpyAsync(host.data(), st->sat_flags, host.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  std::string text;
  for (size_t i = 0; i < host.size(); ++i)
    if (host[i] != 0) {
      ++*n_saturated;
      if (!text.empty()) text += "\n";
      text += st->sat_names[i];
    }
  if (names_cap > 0) {
    const size_t n = std::min((size_t)names_cap - 1, text.size());
    std::memcpy(names, text.data(), n);
    names[n] = '\0';
  }
  if (clear && *n_saturated) HIP_TRY(ctx, hipMemsetAsync(st->sat_flags, 0, host.size() * sizeof(int), s));
  return DITREE_OK;
}

int32_t ditree_profile(ditree_ctx* ctx, int32_t enable) {
  if (!ctx) return DITREE_E_ARG;
  DenoiserState* st = ctx->dn;
  if (!st) return set_err(ctx, DITREE_E_STATE, "profile: weights not loaded");
  st->prof.set(enable);
  return DITREE_OK;
}

int32_t ditree_profile_read(ditree_ctx* ctx, double* ms3, int64_t* launches3, double* flops3) {
  if (!ctx) return DITREE_E_ARG;
  DenoiserState* st = ctx->dn;
  if (!st || !ms3 || !launches3 || !flops3) return set_err(ctx, DITREE_E_STATE, "profile_read: bad state");
  st->prof.collect();
  for (int k = 0; k < 3; ++k) {
    ms3[k] = st->prof.ms_done[k];
    launches3[k] = st->prof.launches_done[k];
    flops3[k] = st->prof.flops_done[k];
  }
  return DITREE_OK;
}

int32_t ditree_denoise_debug_read(ditree_ctx* ctx, const char* name, int32_t B, float* out, int64_t capacity,
                                  int32_t* dims3, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  DenoiserState* st = ctx->dn;
  if (!st || st->prec < 0 || !name || !out || !dims3) return set_err(ctx, DITREE_E_STATE, "debug_read: no workspace");
  hipStream_t s = (hipStream_t)stream;
  std::string nm(name);
  if (nm == "film" || nm == "map_emb") {
    const int cols = nm == "film" ? st->film_cols : st->E;
    const int ld = nm == "film" ? st->film_cols : st->E_ld;
    const float* src = nm == "film" ? st->film : st->map_emb;
    if ((int64_t)B * cols > capacity) return set_err(ctx, DITREE_E_ARG, "debug_read: capacity");
    HIP_TRY(ctx, hipMemcpy2DAsync(out, (size_t)cols * 4, src, (size_t)ld * 4, (size_t)cols * 4, (size_t)B, hipMemcpyDeviceToDevice, s));
    dims3[0] = B; dims3[1] = 1; dims3[2] = cols;
    return DITREE_OK;
  }
  auto it = st->named.find(nm);
  if (it == st->named.end()) return set_err(ctx, DITREE_E_ARG, "debug_read: unknown buffer " + nm);
  const Act& a = it->second;
  if ((int64_t)B * a.L * a.C > capacity) return set_err(ctx, DITREE_E_ARG, "debug_read: capacity");
  launch_unpack_act(a.p, a.ld, a.coff, a.Lp(), a.padded ? 1 : 0, out, B, a.L, a.C, a.fmt, a.plane, s);
  dims3[0] = B; dims3[1] = a.L; dims3[2] = a.C;
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

}  // extern "C"
