// Host tables of libfdm_hip.so (include/fdm_hip.h, fdm_*_host and fdm_model_preset): everything the plan layer derives from
// numbers alone -- diffusion schedules, sampler coefficient tables, ALiBi slopes, the positional table, the windowed-sampling
// layout and blend weights, the table of a slot group, the model presets.  No device, no plan: callable (and tested) on a machine without a GPU.
#include <cmath>

#include "host.hpp"

namespace {
using fdm::fail;

void alibi_slopes(int n, std::vector<double>& out) {       // get_slopes, models/fdm_vocaset.py:96-106
  auto p2 = [](int m, std::vector<double>& o) {
    const double start = std::pow(2.0, -std::pow(2.0, -(std::log2((double)m) - 3.0)));
    for (int i = 0; i < m; ++i) o.push_back(start * std::pow(start, (double)i));
  };
  const double l2 = std::log2((double)n);
  if (l2 == std::floor(l2)) { p2(n, out); return; }
  const int c = 1 << (int)std::floor(l2);
  p2(c, out);
  std::vector<double> more;
  alibi_slopes(2 * c, more);
  for (int i = 0; i < n - c; ++i) out.push_back(more[2 * i]);
}

// cosine_beta_schedule (:537-547) and alphas_cumprod (:565-567) in fp64, in the reference's expression order
void cosine_schedule_f64(int T, std::vector<double>& betas, std::vector<double>& acp) {
  const double s = 0.008;
  std::vector<double> ac(T + 1);
  for (int i = 0; i <= T; ++i) {
    const double c = std::cos((((double)i / T) + s) / (1 + s) * M_PI * 0.5);
    ac[i] = c * c;
  }
  const double a0 = ac[0];
  for (int i = 0; i <= T; ++i) ac[i] = ac[i] / a0;
  betas.resize(T); acp.resize(T);
  double run = 1.0;
  for (int i = 0; i < T; ++i) {
    double b = 1 - (ac[i + 1] / ac[i]);
    b = b < 0 ? 0 : (b > 0.9999 ? 0.9999 : b);
    betas[i] = b;
    run = (i == 0) ? 1.0 - b : run * (1.0 - b);
    acp[i] = run;
  }
}

// times = linspace(-1, T-1, steps+1).astype(int32), ascending (:684-687); numpy: arange(num) * step + start, last = stop
std::vector<int> ddim_time_grid(int steps, int T) {
  std::vector<int> times(steps + 1);
  const double start = -1.0, stop = (double)T - 1.0, step = (stop - start) / steps;
  for (int i = 0; i <= steps; ++i) times[i] = (int)(i == steps ? stop : (double)i * step + start);
  return times;
}

}  // namespace

// Windowed sampling layout (include/fdm_hip.h, fdm_window_layout_host): n windows of W' = min(W, L) frames over L latent frames,
// neighbours overlapping by >= O frames.  L <= W: one window; otherwise n = ceil((L - O) / (W - O)), s_w = floor(w (L - W) / (n - 1)).
int fdm::window_layout(int L, int W, int O, std::vector<int>& starts) {
  if (W < 1 || O < 0 || O >= W) return fail(FDM_ERR_ARG, "window_layout: window %d, overlap %d (need 1 <= window, 0 <= overlap < window)", W, O);
  if (L < 1) return fail(FDM_ERR_SHAPE, "window_layout: L_total = %d latent frames", L);
  starts.clear();
  if (L <= W) { starts.push_back(0); return 1; }
  const int n = (int)(((long long)L - O + (W - O) - 1) / (W - O));
  for (int w = 0; w < n; ++w) starts.push_back((int)((long long)w * (L - W) / (n - 1)));
  return n;
}
// normalised blend weights [n, W'] of that layout: omega_w(f) = min(1, (f - s_w + 0.5) / O, (s_w + W' - f - 0.5) / O), no taper at
// the long clip's first / last frame, O = 0 -> 1; w_hat = omega / (sum of omega over the windows covering f), in double, rounded once
void fdm::window_weights(int L, int W, int O, const std::vector<int>& starts, std::vector<float>& out) {
  const int n = (int)starts.size(), Wf = std::min(W, L);
  std::vector<double> om((size_t)n * Wf), sum(L, 0.0);
  for (int w = 0; w < n; ++w)
    for (int i = 0; i < Wf; ++i) {
      const int f = starts[w] + i;
      double o = 1.0;
      if (O > 0) {
        if (starts[w] > 0) o = std::min(o, (i + 0.5) / O);
        if (starts[w] + Wf < L) o = std::min(o, (Wf - i - 0.5) / O);
      }
      om[(size_t)w * Wf + i] = o;
      sum[f] += o;
    }
  out.resize((size_t)n * Wf);
  for (int w = 0; w < n; ++w)
    for (int i = 0; i < Wf; ++i) out[(size_t)w * Wf + i] = (float)(om[(size_t)w * Wf + i] / sum[starts[w] + i]);
}

extern "C" {

int fdm_window_layout_host(int L_total, int window, int overlap, int* starts, int cap) {
  std::vector<int> st;
  const int n = fdm::window_layout(L_total, window, overlap, st);
  if (n < 0) return n;
  if (starts && cap >= n) std::copy(st.begin(), st.end(), starts);
  return n;
}

int fdm_window_weights_host(int L_total, int window, int overlap, float* w) {
  std::vector<int> st;
  const int n = fdm::window_layout(L_total, window, overlap, st);
  if (n < 0) return n;
  if (w) {
    std::vector<float> wt;
    fdm::window_weights(L_total, window, overlap, st, wt);
    std::copy(wt.begin(), wt.end(), w);
  }
  return n;
}

// Tables of one group of a slot plan (include/fdm_hip.h, fdm_slot_admit_long): the windowed layout with window = the slot capacity,
// each window held by a slot of the caller's list.  The weights are window_weights()'s values themselves.
int fdm_slot_group_table_host(int L_total, int L, int overlap, const int* slots, int n, int* off, int* ent_slot, int* ent_start,
                              float* ent_wt, int cap) {
  if (!slots) return fail(FDM_ERR_ARG, "slot_group_table_host: null slot list");
  std::vector<int> st;
  const int nw = fdm::window_layout(L_total, L, overlap, st);
  if (nw < 0) return nw;
  if (L_total <= L) return fail(FDM_ERR_SHAPE, "slot_group_table_host: L_total = %d fits one slot of %d frames (no group needed)", L_total, L);
  if (n != nw) return fail(FDM_ERR_SHAPE, "slot_group_table_host: %d slots for %d windows", n, nw);
  const long long total = (long long)nw * L;
  if (total > 0x7fffffffLL) return fail(FDM_ERR_SHAPE, "slot_group_table_host: %d windows of %d frames", nw, L);
  if (cap < total || !off || !ent_slot || !ent_start || !ent_wt) return (int)total;
  std::vector<float> wt;
  fdm::window_weights(L_total, L, overlap, st, wt);
  int k = 0;
  off[0] = 0;
  for (int f = 0; f < L_total; ++f) {
    for (int w = 0; w < nw; ++w)
      if (st[w] <= f && f < st[w] + L) { ent_slot[k] = slots[w]; ent_start[k] = st[w]; ent_wt[k] = wt[(size_t)w * L + (f - st[w])]; ++k; }
    off[f + 1] = k;
  }
  return k;
}

int fdm_schedule_host(int T, float* out) {
  if (T <= 0 || !out) return fail(FDM_ERR_ARG, "schedule_host: bad argument");
  // the 12 buffers (:565-603), fp64 in the reference's expression order
  std::vector<double> betas, acp;
  cosine_schedule_f64(T, betas, acp);
  for (int i = 0; i < T; ++i) {
    const double alpha = 1.0 - betas[i], acprev = i ? acp[i - 1] : 1.0;
    const double pv = betas[i] * (1.0 - acprev) / (1.0 - acp[i]);
    const double v[12] = {betas[i], acp[i], acprev, std::sqrt(acp[i]), std::sqrt(1.0 - acp[i]), std::log(1.0 - acp[i]),
                          std::sqrt(1.0 / acp[i]), std::sqrt(1.0 / acp[i] - 1), pv, std::log(pv < 1e-20 ? 1e-20 : pv),
                          betas[i] * std::sqrt(acprev) / (1.0 - acp[i]), (1.0 - acprev) * std::sqrt(alpha) / (1.0 - acp[i])};
    for (int k = 0; k < 12; ++k) out[(size_t)k * T + i] = (float)v[k];
  }
  return FDM_OK;
}

int fdm_ddim_schedule_host(int steps, int T, int* t, int* t_next, float* sqrt_an, float* c_n) {
  if (steps <= 0 || T <= 0) return fail(FDM_ERR_ARG, "ddim_schedule_host: bad argument");
  const std::vector<int> times = ddim_time_grid(steps, T);       // walked from the end, zipped (:684-687)
  std::vector<double> betas, acp;
  if (sqrt_an || c_n) cosine_schedule_f64(T, betas, acp);
  int n = 0;
  for (int i = steps; i >= 1; --i) {
    const int tc = times[i], tn = times[i - 1];
    if (tn < 0) continue;                    // the dead last pair (:695-696)
    if (t) t[n] = tc;
    if (t_next) t_next[n] = tn;
    if (sqrt_an || c_n) {
      const float an = (float)acp[tn];                   // the fp32 alphas_cumprod[t_next] buffer; eta = 0 -> sigma = 0 (:699-708)
      if (sqrt_an) sqrt_an[n] = std::sqrt(an);
      if (c_n) c_n[n] = std::sqrt((1.f - an) - 0.f);
    }
    ++n;
  }
  return n;
}

int fdm_sampler_tables_host(int kind, int steps, int T, double eta, int* t, float* a, float* b, float* c, float* s) {
  if (kind != FDM_SAMPLER_DPMPP_2M && kind != FDM_SAMPLER_DDIM) return fail(FDM_ERR_ARG, "sampler_tables_host: unknown kind %d", kind);
  if (T < 1 || steps < 1 || steps > T) return fail(FDM_ERR_ARG, "sampler_tables_host: steps = %d outside [1, T = %d]", steps, T);
  if (!(eta >= 0.0 && eta <= 1.0)) return fail(FDM_ERR_ARG, "sampler_tables_host: eta = %g outside [0, 1]", eta);
  if (kind == FDM_SAMPLER_DPMPP_2M && eta != 0.0) return fail(FDM_ERR_ARG, "sampler_tables_host: DPM-Solver++ 2M is deterministic (eta must be 0)");
  if (!t || !a || !b || !c || !s) return fail(FDM_ERR_ARG, "sampler_tables_host: null output");
  // the grid of fdm_ddim_schedule_host, every pair executed: the last one, (t_last, -1), goes to data (alpha_bar(-1) := 1);
  // alphas_cumprod stays in fp64 (the values of fdm_schedule_host before its fp32 cast)
  const std::vector<int> times = ddim_time_grid(steps, T);
  std::vector<double> betas, acp;
  cosine_schedule_f64(T, betas, acp);
  double h_prev = 0.0;
  for (int k = 0; k < steps; ++k) {
    const int tc = times[steps - k], tn = times[steps - k - 1];
    t[k] = tc;
    if (tn < 0) { a[k] = 0.f; b[k] = 1.f; c[k] = 0.f; s[k] = 0.f; continue; }
    const double ab = acp[tc], abn = acp[tn];
    if (kind == FDM_SAMPLER_DDIM) {
      const double sg = eta * std::sqrt((1.0 - abn) / (1.0 - ab)) * std::sqrt(1.0 - ab / abn);
      const double av = std::sqrt(1.0 - abn - sg * sg) / std::sqrt(1.0 - ab);
      a[k] = (float)av; b[k] = (float)(std::sqrt(abn) - av * std::sqrt(ab)); c[k] = 0.f; s[k] = (float)sg;
      continue;
    }
    const double lam = 0.5 * std::log(ab / (1.0 - ab)), lam_n = 0.5 * std::log(abn / (1.0 - abn));
    const double h = lam_n - lam, phi = std::sqrt(abn) * (1.0 - std::exp(-h));
    a[k] = (float)(std::sqrt(1.0 - abn) / std::sqrt(1.0 - ab)); s[k] = 0.f;
    if (k == 0) { b[k] = (float)phi; c[k] = 0.f; }
    else { const double r = h_prev / h; b[k] = (float)(phi * (1.0 + 1.0 / (2.0 * r))); c[k] = (float)(-phi / (2.0 * r)); }
    h_prev = h;
  }
  return FDM_OK;
}

int fdm_alibi_slopes_host(int n_head, float* out) {
  if (n_head <= 0 || !out) return fail(FDM_ERR_ARG, "alibi_slopes_host: bad argument");
  std::vector<double> v;
  alibi_slopes(n_head, v);
  for (int i = 0; i < n_head; ++i) out[i] = (float)v[i];
  return FDM_OK;
}

int fdm_pe_table_host(int d, int periodic, int period, int rows, float* out) {
  if (d <= 0 || d % 2 || rows <= 0 || !out || (periodic && period <= 0)) return fail(FDM_ERR_ARG, "pe_table_host: bad argument");
  // pe[p, 2k] = sin(p w_k), pe[p, 2k+1] = cos(p w_k), w_k = exp(2k * (-ln 10000 / d)); periodic: p -> p mod period (:150-184).
  // The reference evaluates these in fp32 torch ops; here each fp32 step is the correctly rounded value of the same function
  // (<= 1 ulp from any fp32 libm); callers that need the reference buffer bit for bit pass "PE.pe" to fdm_plan_set_weights.
  const float coef = (float)(-std::log(10000.0) / d);
  for (int p = 0; p < rows; ++p) {
    const float pos = (float)(periodic ? p % period : p);
    for (int k = 0; k < d; k += 2) {
      const float div = (float)std::exp((double)((float)k * coef));
      const float arg = pos * div;
      out[(size_t)p * d + k] = (float)std::sin((double)arg);
      out[(size_t)p * d + k + 1] = (float)std::cos((double)arg);
    }
  }
  return FDM_OK;
}

// ---- audio front end (include/fdm_hip.h, fdm_frontend_*): ratio, output length and taps of the polyphase resampler to 16 kHz
int fdm_resample_ratio_host(int rate, int* up, int* down) {
  if (rate < 1 || !up || !down) return fail(FDM_ERR_ARG, "resample_ratio_host: rate = %d (or a null output)", rate);
  int a = rate, b = 16000;
  while (b) { const int t = a % b; a = b; b = t; }
  const int u = 16000 / a, d = rate / a;
  if (std::max(u, d) > 2048) return fail(FDM_ERR_SHAPE, "resample_ratio_host: %d Hz -> 16000 Hz is %d / %d (the larger may be at most 2048)", rate, u, d);
  *up = u; *down = d;
  return FDM_OK;
}

long long fdm_resample_len_host(int rate, long long frames) {
  int up = 0, down = 0;
  const int r = fdm_resample_ratio_host(rate, &up, &down);
  if (r != FDM_OK) return r;
  if (frames < 1) return fail(FDM_ERR_SHAPE, "resample_len_host: %lld sample frames", frames);
  if (frames > 0x7fffffffffffffffLL / up - down) return fail(FDM_ERR_SHAPE, "resample_len_host: %lld sample frames overflow 64 bits", frames);
  return (frames * up + down - 1) / down;
}

// scipy.signal.resample_poly's default filter: firwin(2 half + 1, 1 / m, window = ('kaiser', 5.0)) * up with m = max(up, down), half = 10 m
int fdm_resample_taps_host(int up, int down, double* taps) {
  if (up < 1 || down < 1 || !taps) return fail(FDM_ERR_ARG, "resample_taps_host: up = %d, down = %d (or null taps)", up, down);
  const int m = std::max(up, down);
  if (m > 2048) return fail(FDM_ERR_SHAPE, "resample_taps_host: %d / %d (the larger may be at most 2048)", up, down);
  auto i0 = [](double x) {          // modified Bessel function of the first kind, order 0: sum_k ((x / 2)^k / k!)^2
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
      term *= q / ((double)k * (double)k);
      sum += term;
      if (term < 1e-17 * sum) break;
    }
    return sum;
  };
  const int half = 10 * m, n = 2 * half + 1;
  const double fc = 1.0 / m, beta = 5.0, den = i0(beta);
  double total = 0.0;
  for (int k = 0; k < n; ++k) {
    const double t = (double)(k - half), a = fc * t;
    const double sinc = a == 0.0 ? 1.0 : std::sin(M_PI * a) / (M_PI * a);
    const double r = t / half, w = i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / den;
    taps[k] = fc * sinc * w;
    total += taps[k];
  }
  for (int k = 0; k < n; ++k) taps[k] = taps[k] / total * up;
  return n;
}

int fdm_model_preset(const char* name, fdm_model_desc* o) {
  if (!name || !o) return fail(FDM_ERR_ARG, "model_preset: null argument");
  const fdm_model_desc vocaset = {1024, 8, 8, 2048, 16, 64, 8, 0, 1024, 1, 1, 30, 1, 0, 600};
  const fdm_model_desc mead = {512, 4, 8, 1024, 8, 64, 25, 7, 2048, 2, 0, 30, 1, 0, 600};
  const fdm_model_desc biwi = {1024, 4, 8, 2048, 8, 128, 6, 0, 1536, 2, 0, 25, 0, 1, 600};
  const std::string n(name);
  if (n == "vocaset") *o = vocaset;
  else if (n == "mead") *o = mead;
  else if (n == "biwi") *o = biwi;
  else if (n == "vocaset_tiny") { *o = vocaset; o->d = 256; o->n_head = 2; o->n_layers = 2; o->ffn = 512; o->c = 16; }
  else if (n == "mead_tiny") { *o = mead; o->d = 256; o->n_head = 2; o->n_layers = 2; o->ffn = 512; o->c = 32; }
  else return fail(FDM_ERR_ARG, "model_preset: unknown preset '%s'", name);
  return FDM_OK;
}

}  // extern "C"
