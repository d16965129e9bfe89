// Weighted / smoothed loss head (see loss_head.h): k_xent_head / k_xent_rows / k_xent_finish of gemm.hip with
// sample weights, class weights, label smoothing and dense targets as template parameters, in the same two
// forms (one 1024-thread workgroup with the K <= 64 fast path; rows + finish for large heads), the same row
// order and the same f64 sums.  The sparse instantiations without smoothing keep xent_head's expressions
// (loss = lse - z[y], dz = (exp(z - lse) - onehot) * scale), so that no weights or weights of 1 give its
// bits; every instantiation with a sum over the classes in its loss works on the shifted logits u = z - max.
#include "common.h"
#include "loss_head.h"

namespace tdl {

namespace {

// max of a wave's (value, index) pairs, first index on ties (tf.argmax), in every lane
__device__ __forceinline__ void wave_argmax(float& mx, int& am) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o);
    const int oa = __shfl_xor(am, o);
    if (om > mx || (om == mx && oa < am)) {
      mx = om;
      am = oa;
    }
  }
}

// One row by one wave, any K (lane l takes classes l, l + 64, ..): writes the row's dz, returns (in every
// lane) its loss, whether its top-1 class is the target's, and its weight.
template <bool DENSE, bool SW, bool CW, bool EPS>
__device__ __forceinline__ void row_wave(const float* __restrict__ z, const long long* __restrict__ lab,
                                         const float* __restrict__ tgt, const float* __restrict__ sw,
                                         const float* __restrict__ cw, int row, int K, float inv_gn, float ome,
                                         float epk, float* __restrict__ dz, float& loss, float& cor, float& w) {
  const int lane = threadIdx.x & 63;
  const float* zr = z + (long long)row * K;
  float* dr = dz + (long long)row * K;
  float mx = -INFINITY;
  int am = K;
  for (int k = lane; k < K; k += 64) {
    const float v = zr[k];
    if (v > mx) {
      mx = v;
      am = k;
    }
  }
  wave_argmax(mx, am);
  w = SW ? sw[row] : 1.f;
  if (!DENSE) {
    float se = 0.f, su = 0.f;
    for (int k = lane; k < K; k += 64) {
      const float u = zr[k] - mx;
      se += __expf(u);
      if (EPS) su += u;
    }
    se = wave_sum(se);
    const float lg = __logf(se);
    const float lse = mx + lg;
    const long long y = lab[row];
    const bool valid = y >= 0 && y < K;
    if (CW && valid) w = w * cw[y];
    const float scale = (SW || CW) ? w * inv_gn : inv_gn;
    if (EPS) {
      su = wave_sum(su);
      const float qo = valid ? epk : 0.f, qy = valid ? ome + epk : 0.f;  // (an invalid label: q = 0)
      for (int k = lane; k < K; k += 64) dr[k] = (__expf(zr[k] - lse) - (k == y ? qy : qo)) * scale;
      loss = valid ? lg - ome * (zr[y] - mx) - epk * su : 0.f;
    } else {
      for (int k = lane; k < K; k += 64) dr[k] = (__expf(zr[k] - lse) - (k == y ? 1.f : 0.f)) * scale;
      loss = valid ? lse - zr[y] : 0.f;
    }
    cor = (valid && am == (int)y) ? 1.f : 0.f;
  } else {
    const float* tr = tgt + (long long)row * K;
    float tm = -INFINITY;
    int ta = K;
    float se = 0.f, sq = 0.f, squ = 0.f;
    for (int k = lane; k < K; k += 64) {
      const float u = zr[k] - mx, t = tr[k];
      if (t > tm) {
        tm = t;
        ta = k;
      }
      const float q = EPS ? ome * t + epk : t;
      se += __expf(u);
      sq += q;
      squ += q * u;
    }
    wave_argmax(tm, ta);
    se = wave_sum(se);
    sq = wave_sum(sq);
    squ = wave_sum(squ);
    const float lg = __logf(se);
    const float lse = mx + lg;
    if (CW && ta < K) w = w * cw[ta];
    const float scale = (SW || CW) ? w * inv_gn : inv_gn;
    for (int k = lane; k < K; k += 64) {
      const float t = tr[k];
      const float q = EPS ? ome * t + epk : t;
      dr[k] = (__expf(zr[k] - lse) * sq - q) * scale;
    }
    loss = sq * lg - squ;
    cor = (am == ta && ta < K) ? 1.f : 0.f;
  }
}

// One workgroup of 16 waves; wave w takes rows w, w + 16, ..; lane 0 of each wave accumulates its rows in
// row order, thread 0 sums the waves in order (k_xent_head's reduction).
template <bool DENSE, bool SW, bool CW, bool EPS>
__global__ __launch_bounds__(1024) void k_xent_head_w(const float* __restrict__ z, const long long* __restrict__ lab,
                                                      const float* __restrict__ tgt, const float* __restrict__ sw,
                                                      const float* __restrict__ cw, int N, int K, double gn,
                                                      float eps, float* __restrict__ loss_out,
                                                      float* __restrict__ dz, double* lt_total, double* lt_count,
                                                      double* acc_total, double* acc_count) {
  constexpr bool WT = SW || CW;
  __shared__ double s_loss[16], s_cor[16], s_cnt[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float inv_gn = (float)(1.0 / gn);
  const float ome = 1.f - eps, epk = eps / (float)K;
  double my_loss = 0.0, my_cor = 0.0, my_cnt = 0.0;
  // the accumulators' old values, loaded by thread 0 ahead of the rows (only this kernel writes them, in
  // stream order)
  double l0 = 0.0, l1 = 0.0, a0 = 0.0, a1 = 0.0;
  if (threadIdx.x == 0) {
    l0 = lt_total != nullptr ? *lt_total : 0.0;
    l1 = lt_count != nullptr ? *lt_count : 0.0;
    a0 = acc_total != nullptr ? *acc_total : 0.0;
    a1 = acc_count != nullptr ? *acc_count : 0.0;
  }
  if (K <= 64) {
    // a row is one load per lane and column: each wave issues the loads of its next 4 rows (logits, labels or
    // targets, weights) before any math (k_xent_head's small-head path)
    for (int base = w; base < N; base += 64) {
      float v[4], t[4], rw[4];
      long long yy[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = base + 16 * i;
        const bool ok = row < N;
        v[i] = (ok && lane < K) ? z[(long long)row * K + lane] : -INFINITY;
        if (DENSE) {
          t[i] = (ok && lane < K) ? tgt[(long long)row * K + lane] : 0.f;
          yy[i] = -1;
        } else {
          t[i] = 0.f;
          yy[i] = ok ? lab[row] : -1;
        }
        rw[i] = (SW && ok) ? sw[row] : 1.f;
      }
      if (CW && !DENSE) {
#pragma unroll
        for (int i = 0; i < 4; ++i)  // (a label outside [0, K), or a row past N: class weight 1, cw not read)
          if (yy[i] >= 0 && yy[i] < K) rw[i] = rw[i] * cw[yy[i]];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = base + 16 * i;
        if (row >= N) break;  // (wave-uniform)
        float mx = -INFINITY;
        int am = K;
        if (lane < K && v[i] > mx) {
          mx = v[i];
          am = lane;
        }
        wave_argmax(mx, am);
        const float u = lane < K ? v[i] - mx : 0.f;
        float se = lane < K ? __expf(v[i] - mx) : 0.f;
        se = wave_sum(se);
        const float lg = __logf(se);
        const float lse = mx + lg;
        float rloss, rcor, rwt = rw[i];
        if (!DENSE) {
          const long long y = yy[i];
          const bool valid = y >= 0 && y < K;
          const float zy = __shfl(v[i], valid ? (int)y : 0);
          const float scale = WT ? rwt * inv_gn : inv_gn;
          if (EPS) {
            const float su = wave_sum(u);
            const float q = valid ? (lane == y ? ome + epk : epk) : 0.f;
            if (lane < K) dz[(long long)row * K + lane] = (__expf(v[i] - lse) - q) * scale;
            rloss = valid ? lg - ome * (zy - mx) - epk * su : 0.f;
          } else {
            if (lane < K) dz[(long long)row * K + lane] = (__expf(v[i] - lse) - (lane == y ? 1.f : 0.f)) * scale;
            rloss = valid ? lse - zy : 0.f;
          }
          rcor = (valid && am == (int)y) ? 1.f : 0.f;
        } else {
          float tm = -INFINITY;
          int ta = K;
          if (lane < K && t[i] > tm) {
            tm = t[i];
            ta = lane;
          }
          wave_argmax(tm, ta);
          const float q = lane < K ? (EPS ? ome * t[i] + epk : t[i]) : 0.f;
          const float sq = wave_sum(q);
          const float squ = wave_sum(q * u);
          if (CW && ta < K) rwt = rwt * cw[ta];
          const float scale = WT ? rwt * inv_gn : inv_gn;
          if (lane < K) dz[(long long)row * K + lane] = (__expf(v[i] - lse) * sq - q) * scale;
          rloss = sq * lg - squ;
          rcor = (am == ta && ta < K) ? 1.f : 0.f;
        }
        if (lane == 0) {
          if (WT) {
            my_loss += (double)rwt * (double)rloss;
            my_cor += (double)rwt * (double)rcor;
            my_cnt += (double)rwt;
          } else {
            my_loss += (double)rloss;
            my_cor += (double)rcor;
          }
        }
      }
    }
  }
  for (int row = K <= 64 ? N : w; row < N; row += 16) {
    float rloss, rcor, rwt;
    row_wave<DENSE, SW, CW, EPS>(z, lab, tgt, sw, cw, row, K, inv_gn, ome, epk, dz, rloss, rcor, rwt);
    if (lane == 0) {
      if (WT) {
        my_loss += (double)rwt * (double)rloss;
        my_cor += (double)rwt * (double)rcor;
        my_cnt += (double)rwt;
      } else {
        my_loss += (double)rloss;
        my_cor += (double)rcor;
      }
    }
  }
  if (lane == 0) {
    s_loss[w] = my_loss;
    s_cor[w] = my_cor;
    s_cnt[w] = my_cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tl = 0.0, tc = 0.0, tn = 0.0;
    for (int i = 0; i < 16; ++i) {
      tl += s_loss[i];
      tc += s_cor[i];
      tn += s_cnt[i];
    }
    loss_out[0] = (float)(tl / gn);
    if (lt_total != nullptr) *lt_total = l0 + tl;
    if (lt_count != nullptr) *lt_count = l1 + (double)N;
    if (acc_total != nullptr) *acc_total = a0 + tc;
    if (acc_count != nullptr) *acc_count = a1 + (WT ? tn : (double)N);
  }
}

// Large heads: one wave per row over many workgroups writes the row's loss, correct flag, weight and dz;
// k_xent_finish_w (one workgroup) sums the rows in a fixed order.
template <bool DENSE, bool SW, bool CW, bool EPS>
__global__ __launch_bounds__(256) void k_xent_rows_w(const float* __restrict__ z, const long long* __restrict__ lab,
                                                     const float* __restrict__ tgt, const float* __restrict__ sw,
                                                     const float* __restrict__ cw, int N, int K, double gn, float eps,
                                                     float* __restrict__ dz, float* __restrict__ row_loss,
                                                     float* __restrict__ row_cor, float* __restrict__ row_w) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float inv_gn = (float)(1.0 / gn);
  const float ome = 1.f - eps, epk = eps / (float)K;
  float rloss, rcor, rwt;
  row_wave<DENSE, SW, CW, EPS>(z, lab, tgt, sw, cw, row, K, inv_gn, ome, epk, dz, rloss, rcor, rwt);
  if ((threadIdx.x & 63) == 0) {
    row_loss[row] = rloss;
    row_cor[row] = rcor;
    if (SW || CW) row_w[row] = rwt;
  }
}

template <bool WT>
__global__ __launch_bounds__(1024) void k_xent_finish_w(const float* __restrict__ row_loss,
                                                        const float* __restrict__ row_cor,
                                                        const float* __restrict__ row_w, int N, double gn,
                                                        float* __restrict__ loss_out, double* lt_total,
                                                        double* lt_count, double* acc_total, double* acc_count) {
  __shared__ double s_l[1024], s_c[1024], s_n[1024];
  const int t = threadIdx.x;
  double l = 0.0, c = 0.0, n = 0.0;
  for (int r = t; r < N; r += 1024) {  // (each thread its rows in order, then a fixed tree)
    if (WT) {
      const double wr = (double)row_w[r];
      l += wr * (double)row_loss[r];
      c += wr * (double)row_cor[r];
      n += wr;
    } else {
      l += (double)row_loss[r];
      c += (double)row_cor[r];
    }
  }
  s_l[t] = l;
  s_c[t] = c;
  s_n[t] = n;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (t < w) {
      s_l[t] += s_l[t + w];
      s_c[t] += s_c[t + w];
      s_n[t] += s_n[t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double tl = s_l[0], tc = s_c[0], tn = s_n[0];
    loss_out[0] = (float)(tl / gn);
    const double l0 = lt_total != nullptr ? *lt_total : 0.0, l1 = lt_count != nullptr ? *lt_count : 0.0;
    const double a0 = acc_total != nullptr ? *acc_total : 0.0, a1 = acc_count != nullptr ? *acc_count : 0.0;
    if (lt_total != nullptr) *lt_total = l0 + tl;
    if (lt_count != nullptr) *lt_count = l1 + (double)N;
    if (acc_total != nullptr) *acc_total = a0 + tc;
    if (acc_count != nullptr) *acc_count = a1 + (WT ? tn : (double)N);
  }
}

struct HeadArgs {
  const float* z;
  const long long* labels;
  const float* targets;
  const float* sw;
  const float* cw;
  int N, K;
  double gn;
  float eps;
  float* loss_out;
  float* dz;
  double *lt_total, *lt_count, *acc_total, *acc_count;
  float* ws;
  hipStream_t s;
};

template <bool DENSE, bool SW, bool CW, bool EPS>
void launch(const HeadArgs& a) {
  if (a.ws == nullptr) {
    hipLaunchKernelGGL((k_xent_head_w<DENSE, SW, CW, EPS>), dim3(1), dim3(1024), 0, a.s, a.z, a.labels, a.targets,
                       a.sw, a.cw, a.N, a.K, a.gn, a.eps, a.loss_out, a.dz, a.lt_total, a.lt_count, a.acc_total,
                       a.acc_count);
    return;
  }
  float *rl = a.ws, *rc = a.ws + a.N, *rw = a.ws + 2 * (long long)a.N;
  if (a.N > 0)  // (no rows: the finish alone writes a zero loss and leaves the sums as they are)
    hipLaunchKernelGGL((k_xent_rows_w<DENSE, SW, CW, EPS>), dim3((a.N + 3) / 4), dim3(256), 0, a.s, a.z, a.labels,
                       a.targets, a.sw, a.cw, a.N, a.K, a.gn, a.eps, a.dz, rl, rc, rw);
  hipLaunchKernelGGL((k_xent_finish_w<SW || CW>), dim3(1), dim3(1024), 0, a.s, rl, rc, rw, a.N, a.gn, a.loss_out,
                     a.lt_total, a.lt_count, a.acc_total, a.acc_count);
}

template <bool DENSE, bool SW, bool CW>
void pick_eps(const HeadArgs& a) {
  if (a.eps != 0.f)
    launch<DENSE, SW, CW, true>(a);
  else
    launch<DENSE, SW, CW, false>(a);
}

template <bool DENSE>
void pick_weights(const HeadArgs& a) {
  if (a.sw != nullptr && a.cw != nullptr)
    pick_eps<DENSE, true, true>(a);
  else if (a.sw != nullptr)
    pick_eps<DENSE, true, false>(a);
  else if (a.cw != nullptr)
    pick_eps<DENSE, false, true>(a);
  else
    pick_eps<DENSE, false, false>(a);
}

}  // namespace

void xent_head_w(const float* z, const long long* labels, const float* targets, const float* sw, const float* cw,
                 int N, int K, double gn, float eps, float* loss_out, float* dz, double* lt_total, double* lt_count,
                 double* acc_total, double* acc_count, float* rows_ws, hipStream_t s) {
  const HeadArgs a{z, labels, targets, sw, cw, N, K, gn, eps, loss_out, dz, lt_total, lt_count, acc_total, acc_count,
                   rows_ws, s};
  if (targets != nullptr)
    pick_weights<true>(a);
  else
    pick_weights<false>(a);
}

// k_gather_xy (ops.hip) with the row's f32 weight as a third column
__global__ __launch_bounds__(256) void k_gather_xyw(const float* __restrict__ src, const void* __restrict__ lab,
                                                    const float* __restrict__ wt, const int* __restrict__ idx,
                                                    float* __restrict__ out, void* __restrict__ out_lab,
                                                    float* __restrict__ out_w, int64_t row_elems, int lab_bytes) {
  const int64_t r = blockIdx.x;
  const int64_t i = idx[r];
  const float* s = src + i * row_elems;
  float* o = out + r * row_elems;
  if ((row_elems & 3) == 0) {
    for (int64_t e = threadIdx.x * 4; e < row_elems; e += 1024) st4(o + e, ld4(s + e));
  } else {
    for (int64_t e = threadIdx.x; e < row_elems; e += 256) o[e] = s[e];
  }
  if (threadIdx.x == 0) {
    if (lab_bytes == 8)
      static_cast<long long*>(out_lab)[r] = static_cast<const long long*>(lab)[i];
    else
      static_cast<int*>(out_lab)[r] = static_cast<const int*>(lab)[i];
    out_w[r] = wt[i];
  }
}

void gather_xyw(const float* src, const void* lab, const float* w, const int* idx, float* out, void* out_lab,
                float* out_w, int64_t rows, int64_t row_elems, int lab_bytes, hipStream_t s) {
  if (rows == 0) return;
  hipLaunchKernelGGL(k_gather_xyw, dim3((unsigned)rows), dim3(256), 0, s, src, lab, w, idx, out, out_lab, out_w,
                     row_elems, lab_bytes);
}

}  // namespace tdl
