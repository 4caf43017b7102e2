// k_assemble_fused.hip — assembly and the kept list's first step in one launch
// (k_assemble.hip's per-span code with k_util.hip's kept_compact_block /
// KeptTile). Included by api.hip (unity build), at global scope after
// `using namespace tsdb`.
#pragma once

// Groups of up to 1024 spans: the assembly (thread per span, then the
// deferred spans a wave each) and the kept-list compaction in one 1024-thread
// block, one launch instead of three.
__global__ void __launch_bounds__(1024) k_assemble_small(AssembleArgs a, KeptArgs K) {
  __shared__ uint32_t s_list[1024];
  __shared__ uint32_t s_n;
  const uint32_t t = threadIdx.x;
  if (t == 0) s_n = 0;
  __syncthreads();
  if (t < a.n_spans && assemble_fast_one(a, t)) s_list[atomicAdd(&s_n, 1u)] = t;
  __syncthreads();
  const uint32_t nd = s_n;
  for (uint32_t w = t / WAVE; w < nd; w += 1024 / WAVE) assemble_span_wave(a, s_list[w]);
  __syncthreads();  // (the block's global writes visible to the whole block)
  kept_compact_block(K);
}

// Groups of (nearly) single-row spans beyond one block (rows <= 2 x spans:
// C3's 1M series): a tile of 256 spans assembled (a thread a span, the
// block's waves walking the deferred ones, as k_assemble_small) and its kept
// sums in one launch, instead of k_assemble_fast, k_assemble and
// k_kept_tiles. The sums of the tile travel as one wave-reduced row per wave
// through LDS (one barrier).
__global__ void __launch_bounds__(256) k_assemble_tiles(AssembleArgs a, KeptTile* tile_sum, ulonglong2* tile_ke) {
  __shared__ uint32_t s_list[256];
  __shared__ uint32_t s_n;
  __shared__ uint64_t s_r[4][11];
  const uint32_t t = threadIdx.x, lane = lane_id(), w = t / WAVE;
  const uint32_t s = blockIdx.x * 256 + t;
  if (t == 0) s_n = 0;
  __syncthreads();
  if (s < a.n_spans && assemble_fast_one(a, s)) s_list[atomicAdd(&s_n, 1u)] = s;
  __syncthreads();
  const uint32_t nd = s_n;
  for (uint32_t i = w; i < nd; i += 256 / WAVE) assemble_span_wave(a, s_list[i]);
  if (nd) __syncthreads();  // (the block's global writes visible to the whole block)
  uint64_t sk = 0, se = 0, cnt = 0;
  int64_t f = INT64_MAX, l = INT64_MIN, fx = INT64_MIN, ln = INT64_MAX;
  UKeyAcc u;
  u.init();
  if (s < a.n_spans) {
    se = a.sp_cap[s];
    if (a.sp_kept[s]) {
      sk = 1;
      cnt = a.sp_ncells[s];
      f = fx = a.sp_first[s];
      l = ln = a.sp_last[s];
      if (a.u_key1) u.add(a.u_key1[s], a.u_key2[s]);
    }
  }
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) {
    sk += shfl_xor_u64(sk, m);
    se += shfl_xor_u64(se, m);
    cnt += shfl_xor_u64(cnt, m);
    f = min(f, (int64_t)shfl_xor_u64((uint64_t)f, m));
    l = max(l, (int64_t)shfl_xor_u64((uint64_t)l, m));
    fx = max(fx, (int64_t)shfl_xor_u64((uint64_t)fx, m));
    ln = min(ln, (int64_t)shfl_xor_u64((uint64_t)ln, m));
  }
  if (a.u_key1) u.wave_reduce();
  if (lane == 0) {
    uint64_t* r = s_r[w];
    r[0] = sk; r[1] = se; r[2] = cnt; r[3] = (uint64_t)f; r[4] = (uint64_t)l; r[5] = (uint64_t)fx; r[6] = (uint64_t)ln;
    r[7] = u.a0; r[8] = u.a1; r[9] = u.b0; r[10] = u.b1;
  }
  __syncthreads();
  if (t == 0) {
    for (int i = 1; i < 4; i++) {
      const uint64_t* r = s_r[i];
      sk += r[0]; se += r[1]; cnt += r[2];
      f = min(f, (int64_t)r[3]); l = max(l, (int64_t)r[4]); fx = max(fx, (int64_t)r[5]); ln = min(ln, (int64_t)r[6]);
      u.a0 = min(u.a0, r[7]); u.a1 = max(u.a1, r[8]); u.b0 = min(u.b0, r[9]); u.b1 = max(u.b1, r[10]);
    }
    KeptTile o;
    o.k = sk; o.e = se; o.cnt = cnt; o.pad = 0;
    o.f = cnt ? f : INT64_MAX; o.l = cnt ? l : INT64_MIN; o.fx = cnt ? fx : INT64_MIN; o.ln = cnt ? ln : INT64_MAX;
    o.u = u;
    tile_sum[blockIdx.x] = o;
    tile_ke[blockIdx.x] = make_ulonglong2(sk, se);
  }
}
