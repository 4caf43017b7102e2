// k_ug_ds_reg.hip — the aligned group's finish (k_fap_*) and the hot kernel
// k_ug_ds_reg: k_ds_reg.hip's bodies with the group's tail in the launch's
// last block. Included by api.hip (unity build), at global scope after
// `using namespace tsdb` and k_callstate.hip.
#pragma once

// ---- the optimistic aligned-group finish (no host round trip after the
// grid when the group turns out aligned; see spangroup_run) ----
// this rank's partials stand: every kept span in the one class, G its bucket
// sequence of at most 64 points, no float, no error
// (one thread; then, sharded, the agreement header packed for the group)
// (a whole wave: lane i packs field i; the validity is this wave's own value,
// not re-read from the call state)
DEVI void fap_valid_pack(Small* sm, uint32_t fap_ran, const XMove& pack, uint64_t T) {
  const bool v = fap_ran && sm->err == ERR_NONE && !sm->fap_broken && sm->fap_key[0] == sm->fap_key[1] &&
                 sm->fap_key[2] == sm->fap_key[3] && T > 0 && T <= WAVE && sm->gflags[0] == 0;
  const uint32_t lane = lane_id();
  if (lane == 0) sm->fap_valid = v ? 1ull : 0ull;
  if (lane < pack.n) {
    if (pack.field[lane] == (void*)&sm->fap_valid) pack.buf[lane] = v ? 1ull : 0ull;  // (kind 0: MIN, as is)
    else xmove_one(pack, lane);
  }
}
// this rank's 64-slot partials (k_fap_final64's reduce), its validity, the pack
template <int OP>
__global__ void __launch_bounds__(1024) k_fap_final64v(const int64_t* tmp, uint32_t n, uint32_t n_kept, int64_t* p_i,
                                                       uint32_t* p_cnt, Small* sm, XMove pack) {
  __shared__ int64_t s[16][WAVE];
  const int lane = lane_id();
  const uint32_t w = threadIdx.x / WAVE;
  int64_t acc = fap_rows_wave<OP>(tmp, w, 16, n);
  acc = fap_block_comb<OP>(acc, s);
  if (w == 0) {
    const uint64_t T = *(volatile const uint64_t*)&sm->T;
    const bool in = (uint64_t)lane < T;
    p_i[lane] = in ? acc : fap_neutral(OP);
    p_cnt[lane] = in ? n_kept : 0u;
    fap_valid_pack(sm, 1u, pack, T);
  }
}
// a rank without an aligned-group attempt: neutral partials for the exchange
__global__ void k_fap_neutral64(int64_t* p_i, uint32_t* p_cnt, int op, Small* sm, XMove pack) {
  p_i[threadIdx.x] = fap_neutral(op);
  p_cnt[threadIdx.x] = 0;
  fap_valid_pack(sm, 0u, pack, 0);
}
// The finalize of the (exchanged) 64-slot partials when the group stands
// everywhere (sharded: and every rank's grid is the global one; outputs at a
// fixed stride of 64: ts | bits | is_int), then k_call_end's `done` variant,
// in one block of 256 threads: the call state is snapshot, and reset with
// the bitmap cleared iff the group stood
template <int AGG>
__global__ void __launch_bounds__(256) k_fap_finish_end(Small* sm, const int64_t* p_i, const uint32_t* p_cnt,
                                                        FinalArgs f, int32_t sharded, XMove unpack, Small* snap,
                                                        const Small* init, uint32_t* bitmap, const uint32_t* grid, int64_t lo,
                                                        uint64_t seq) {
  __shared__ uint32_t s_ok, s_T;
  const uint32_t t = threadIdx.x;
  if (t < unpack.n) xmove_one(unpack, t);  // the agreed header back into the call state (sharded), a field a thread
  __syncthreads();
  if (t == 0) {
    bool ok = sm->fap_valid != 0 && sm->err == ERR_NONE && sm->gflags[0] == 0 && sm->T > 0 && sm->T <= WAVE;
    // (sharded: rank-independent: an empty grid anywhere makes lo's MIN / MAX
    // differ, ~0 vs a real lo; all empty fails T > 0 on every rank)
    if (sharded) ok = ok && xh_grids_agree(sm->xh);
    s_ok = ok ? 1u : 0u;
    s_T = (uint32_t)sm->T;
  }
  __syncthreads();
  if (!s_ok) {  // the group did not stand: the state stays for the usual path
    small_snap(sm, snap, nullptr, seq);
    return;
  }
  if (t < s_T) {
    Acc a;
    acc_init(a);
    a.cnt = p_cnt[t];
    a.ia = p_i[t];
    finalize_one<AGG, MODE_INT, false>(f, t, a);
  }
  __syncthreads();
  if (t == 0) sm->fap_done = 1;
  __syncthreads();
  small_snap(sm, snap, init, seq);
  __syncthreads();  // (the grid read below is this block's own)
  if (bitmap && t < s_T) bitmap[(uint64_t)((int64_t)grid[t] - lo) >> 5] = 0u;
}

// ---- the uniform path's aligned group in one launch (uniform_run) ----
// k_ds_reg's body with each block's 64 bucket partials combined by device
// atomics into one of `ncopy` copies (neutral on entry), then the tail in the
// launch's last block (the blocks count themselves done on Small.ug_done
// after their atomics are acknowledged): the copies combined (and reset), G
// from the class key (bucket b of every span: t0 + b kk step +
// floor(step (m_b - 1) / 2) over its m_b cells, Span.java:377-422), the
// group's validity; unsharded, also k_fap_finish_end's finish (the results
// into mapped host memory, the state snapshot + reset + stamp); sharded, the
// 64-slot partials and the agreement header for the exchange, the finish
// after it. One launch for k_ds_reg + k_fap_rows + k_fap_final64v
// (+ k_fap_finish_end).
constexpr uint32_t UG_NCOPY = 16;  // (4 a thread of the tail, loaded together)
struct UgTail {
  Small* sm;
  int op;        // the block combine (0 wrapping add, 1 min, 2 max)
  int agg;       // the cross-series aggregator (finalize)
  int32_t sharded;
  uint32_t n_kept, t0, step, kk, ncell, nb;
  uint32_t* grid;    // G (<= 64 points)
  int64_t* p_i;      // (sharded) the 64-slot partials for the exchange
  uint32_t* p_cnt;
  XMove pack;        // (sharded) the agreement header
  FinalArgs fo;      // (unsharded) the results into mapped host memory
  Small* snap;
  const Small* init;
  uint64_t seq;
  // (speculative, unsharded: the key, n_kept, kk and nb come from the call
  // state; a group that is not one leaves the state as the host would find it)
  uint32_t spec;
  int64_t interval;
};
template <typename T>
DEVI T coherent_load(const T* p) {  // (past any stale L2 line: the other blocks wrote by atomics)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the tail of the launch the host sized (the key, n_kept, kk and nb in UgTail)
DEVI void ug_fap_tail(const FapArgs& fap, const UgTail& t) {
  __shared__ int64_t s_acc[4][WAVE];
  const uint32_t tid = threadIdx.x, lane = tid % WAVE, w = tid / WAVE;
  const int op = t.op;
  const int64_t neutral = fap_neutral(op);
  auto comb = [&](int64_t x, int64_t y) { return op == 0 ? ladd(x, y) : (op == 1 ? min(x, y) : max(x, y)); };
  int64_t acc = neutral;
  {  // (coherent loads, all in flight together; the copies reset to neutral after)
    int64_t v[UG_NCOPY / 4];
#pragma unroll
    for (uint32_t i = 0; i < UG_NCOPY / 4; i++)
      v[i] = (int64_t)coherent_load(fap.copies + (uint64_t)(w + 4 * i) * WAVE + lane);
#pragma unroll
    for (uint32_t i = 0; i < UG_NCOPY / 4; i++) {
      acc = comb(acc, v[i]);
      fap.copies[(uint64_t)(w + 4 * i) * WAVE + lane] = (unsigned long long)neutral;
    }
  }
  s_acc[w][lane] = acc;
  __syncthreads();
  Small* sm = t.sm;
  __shared__ uint32_t s_ok;
  if (w == 0) {
    acc = comb(comb(s_acc[0][lane], s_acc[1][lane]), comb(s_acc[2][lane], s_acc[3][lane]));
    const bool in = lane < t.nb;
    if (in) {
      const uint32_t sb = lane * t.kk, m = min(sb + t.kk, t.ncell) - sb;
      t.grid[lane] = t.t0 + sb * t.step + (uint32_t)((uint64_t)t.step * (m - 1) / 2);
    }
    const bool v = coherent_load(&sm->err) == ERR_NONE && !coherent_load(&sm->fap_broken) &&
                   coherent_load(&sm->fap_key[0]) == coherent_load(&sm->fap_key[1]) &&
                   coherent_load(&sm->fap_key[2]) == coherent_load(&sm->fap_key[3]) && t.nb > 0 && t.nb <= WAVE &&
                   coherent_load(&sm->gflags[0]) == 0;
    if (lane == 0) {
      sm->T = t.nb;
      sm->fap_valid = v ? 1ull : 0ull;
      s_ok = v ? 1u : 0u;
    }
    if (t.sharded) {
      t.p_i[lane] = in ? acc : neutral;
      t.p_cnt[lane] = in ? t.n_kept : 0u;
      if (lane < t.pack.n) {
        if (t.pack.field[lane] == (void*)&sm->fap_valid) t.pack.buf[lane] = v ? 1ull : 0ull;
        else xmove_one(t.pack, lane);
      }
    } else if (v && in) {
      Acc a;
      acc_init(a);
      a.cnt = t.n_kept;
      a.ia = acc;
      switch (t.agg) {
        case 1: finalize_one<1, MODE_INT, false>(t.fo, lane, a); break;
        case 2: finalize_one<2, MODE_INT, false>(t.fo, lane, a); break;
        case 3: finalize_one<3, MODE_INT, false>(t.fo, lane, a); break;
        default: finalize_one<0, MODE_INT, false>(t.fo, lane, a); break;
      }
    }
  }
  __syncthreads();
  if (t.sharded) return;
  // the finish: the results written, the state snapshot and, when the group
  // stood, reset (the host reads fap_done; else the general path runs)
  if (s_ok && tid == 0) sm->fap_done = 1;
  __syncthreads();
  small_snap(sm, t.snap, s_ok ? t.init : nullptr, t.seq);
}
// the speculative launch's tail (sharded): the verdict, key and counts from
// the call state
DEVI void ug_fap_tail_spec(const FapArgs& fap, const UgTail& t) {
  __shared__ int64_t s_acc[4][WAVE];
  const uint32_t tid = threadIdx.x, lane = tid % WAVE, w = tid / WAVE;
  // (the key's fields as locals: a copy of the UgTail, whose pack arrays are
  // indexed by lane, put the whole struct in scratch — 928 B a lane, the
  // launch 3x slower)
  uint32_t n_kept = t.n_kept, t0 = t.t0, step = t.step, kk0 = t.kk, ncell = t.ncell, nbk = t.nb;
  bool fits = true;
  if (t.spec) {
    Small* sm = t.sm;
    uint32_t nb = 0, kk = 0;
    fits = sm->ug_go != 0;
    ug_spec_fits(sm->ukey[0], sm->ukey[1], sm->ukey[2], sm->ukey[3], sm->n_kept, sm->err, t.interval, &nb, &kk);
    // (not one: this rank's partials neutral, its validity 0, as
    // k_fap_neutral64's; the exchange is every rank's)
    n_kept = fits ? (uint32_t)sm->n_kept : 0u;
    t0 = (uint32_t)(sm->ukey[0] >> 32);
    ncell = (uint32_t)sm->ukey[0];
    step = (uint32_t)(sm->ukey[2] >> 32);
    kk0 = fits ? kk : 1u;
    nbk = fits ? nb : 0u;
    if (tid == 0) sm->ug_tried = 1;
  }
  const int op = t.op;
  const int64_t neutral = fap_neutral(op);
  auto comb = [&](int64_t x, int64_t y) { return op == 0 ? ladd(x, y) : (op == 1 ? min(x, y) : max(x, y)); };
  int64_t acc = neutral;
  {  // (coherent loads, all in flight together; the copies reset to neutral after)
    int64_t v[UG_NCOPY / 4];
#pragma unroll
    for (uint32_t i = 0; i < UG_NCOPY / 4; i++)
      v[i] = (int64_t)coherent_load(fap.copies + (uint64_t)(w + 4 * i) * WAVE + lane);
#pragma unroll
    for (uint32_t i = 0; i < UG_NCOPY / 4; i++) {
      acc = comb(acc, v[i]);
      fap.copies[(uint64_t)(w + 4 * i) * WAVE + lane] = (unsigned long long)neutral;
    }
  }
  s_acc[w][lane] = acc;
  __syncthreads();
  Small* sm = t.sm;
  __shared__ uint32_t s_ok;
  if (w == 0) {
    acc = comb(comb(s_acc[0][lane], s_acc[1][lane]), comb(s_acc[2][lane], s_acc[3][lane]));
    const bool in = lane < nbk;
    if (in) {
      const uint32_t sb = lane * kk0, m = min(sb + kk0, ncell) - sb;
      t.grid[lane] = t0 + sb * step + (uint32_t)((uint64_t)step * (m - 1) / 2);
    }
    const bool v = coherent_load(&sm->err) == ERR_NONE && !coherent_load(&sm->fap_broken) &&
                   coherent_load(&sm->fap_key[0]) == coherent_load(&sm->fap_key[1]) &&
                   coherent_load(&sm->fap_key[2]) == coherent_load(&sm->fap_key[3]) && nbk > 0 && nbk <= WAVE &&
                   coherent_load(&sm->gflags[0]) == 0;
    if (lane == 0) {
      sm->T = nbk;
      sm->fap_valid = v ? 1ull : 0ull;
      s_ok = v ? 1u : 0u;
    }
    if (t.sharded) {
      t.p_i[lane] = in ? acc : neutral;
      t.p_cnt[lane] = in ? n_kept : 0u;
      if (lane < t.pack.n) {
        if (t.pack.field[lane] == (void*)&sm->fap_valid) {
          t.pack.buf[lane] = v ? 1ull : 0ull;
        } else if (t.spec && (lane == 4 || lane == 5 || lane == 10 || lane == 11)) {
          // (speculative: the class key's header words, uniform_run's fx[4, 5,
          // 10, 11], from the device key — ~0 / 0 for a rank without a group)
          const uint64_t a1 = fits ? sm->ukey[0] : ~0ull, a2 = fits ? sm->ukey[2] : 0ull;
          const uint64_t val = (lane == 4 || lane == 10) ? a1 : a2;
          t.pack.buf[lane] = t.pack.kind[lane] == 4 ? ~val : val;
        } else {
          xmove_one(t.pack, lane);
        }
      }
    } else if (v && in) {
      Acc a;
      acc_init(a);
      a.cnt = n_kept;
      a.ia = acc;
      switch (t.agg) {
        case 1: finalize_one<1, MODE_INT, false>(t.fo, lane, a); break;
        case 2: finalize_one<2, MODE_INT, false>(t.fo, lane, a); break;
        case 3: finalize_one<3, MODE_INT, false>(t.fo, lane, a); break;
        default: finalize_one<0, MODE_INT, false>(t.fo, lane, a); break;
      }
    }
  }
  __syncthreads();
  if (t.sharded) return;
  // the finish: the results written, the state snapshot and, when the group
  // stood, reset (the host reads fap_done; else the general path runs)
  if (s_ok && tid == 0) sm->fap_done = 1;
  __syncthreads();
  small_snap(sm, t.snap, s_ok ? t.init : nullptr, t.seq);
}
// the direct launch's tail (ds_reg_direct_body: no assembly ran): the class
// key, the verdict, kk and nb from the call state's fap_key; what assembly and
// the kept list would have published (every span kept: n_kept, n_input) is
// written here when the group is one. A sibling of ug_fap_tail_spec, not a
// mode of it or of ug_fap_tail (see k_ug_ds_reg on folding tails).
DEVI void ug_fap_tail_direct(const FapArgs& fap, const UgTail& t) {
  __shared__ int64_t s_acc[4][WAVE];
  const uint32_t tid = threadIdx.x, lane = tid % WAVE, w = tid / WAVE;
  Small* sm = t.sm;
  const unsigned long long k1 = coherent_load(&sm->fap_key[0]), k2 = coherent_load(&sm->fap_key[2]);
  // (one class, every span in it; else this rank's partials neutral and its
  // validity 0, as k_fap_neutral64's)
  const bool one = !coherent_load(&sm->fap_broken) && k1 == coherent_load(&sm->fap_key[1]) &&
                   k2 == coherent_load(&sm->fap_key[3]) && (k2 >> 32) != 0;
  const uint32_t t0 = (uint32_t)(k1 >> 32), ncell = (uint32_t)k1, step = (uint32_t)(k2 >> 32);
  const uint32_t n_kept = one ? t.n_kept : 0u;
  const uint32_t kk0 = one ? (uint32_t)((t.interval + step - 1) / step) : 1u;
  const uint32_t nbk = one ? (ncell + kk0 - 1) / kk0 : 0u;
  const int op = t.op;
  const int64_t neutral = fap_neutral(op);
  auto comb = [&](int64_t x, int64_t y) { return op == 0 ? ladd(x, y) : (op == 1 ? min(x, y) : max(x, y)); };
  int64_t acc = neutral;
  {  // (coherent loads, all in flight together; the copies reset to neutral after)
    int64_t v[UG_NCOPY / 4];
#pragma unroll
    for (uint32_t i = 0; i < UG_NCOPY / 4; i++)
      v[i] = (int64_t)coherent_load(fap.copies + (uint64_t)(w + 4 * i) * WAVE + lane);
#pragma unroll
    for (uint32_t i = 0; i < UG_NCOPY / 4; i++) {
      acc = comb(acc, v[i]);
      fap.copies[(uint64_t)(w + 4 * i) * WAVE + lane] = (unsigned long long)neutral;
    }
  }
  s_acc[w][lane] = acc;
  __syncthreads();
  __shared__ uint32_t s_ok;
  if (w == 0) {
    acc = comb(comb(s_acc[0][lane], s_acc[1][lane]), comb(s_acc[2][lane], s_acc[3][lane]));
    const bool in = lane < nbk;
    if (in) {
      const uint32_t sb = lane * kk0, m = min(sb + kk0, ncell) - sb;
      t.grid[lane] = t0 + sb * step + (uint32_t)((uint64_t)step * (m - 1) / 2);
    }
    const bool v = one && coherent_load(&sm->err) == ERR_NONE && nbk > 0 && nbk <= WAVE &&
                   coherent_load(&sm->gflags[0]) == 0;
    if (lane == 0) {
      sm->T = nbk;
      sm->fap_valid = v ? 1ull : 0ull;
      s_ok = v ? 1u : 0u;
      if (one) {  // (the kept-list kernel's counts: every span kept, n cells each)
        sm->n_kept = n_kept;
        sm->n_input = (unsigned long long)n_kept * ncell;
      }
    }
    if (t.sharded) {
      t.p_i[lane] = in ? acc : neutral;
      t.p_cnt[lane] = in ? n_kept : 0u;
      if (lane < t.pack.n) {
        if (t.pack.field[lane] == (void*)&sm->fap_valid) {
          t.pack.buf[lane] = v ? 1ull : 0ull;
        } else if (lane == 4 || lane == 5 || lane == 10 || lane == 11) {
          // (the class key's header words, as the speculative tail's: ~0 / 0
          // for a rank without a group)
          const uint64_t a1 = one ? k1 : ~0ull, a2 = one ? k2 : 0ull;
          const uint64_t val = (lane == 4 || lane == 10) ? a1 : a2;
          t.pack.buf[lane] = t.pack.kind[lane] == 4 ? ~val : val;
        } else {
          xmove_one(t.pack, lane);
        }
      }
    } else if (v && in) {
      Acc a;
      acc_init(a);
      a.cnt = n_kept;
      a.ia = acc;
      switch (t.agg) {
        case 1: finalize_one<1, MODE_INT, false>(t.fo, lane, a); break;
        case 2: finalize_one<2, MODE_INT, false>(t.fo, lane, a); break;
        case 3: finalize_one<3, MODE_INT, false>(t.fo, lane, a); break;
        default: finalize_one<0, MODE_INT, false>(t.fo, lane, a); break;
      }
    }
  }
  __syncthreads();
  if (t.sharded) return;
  // the finish, as ug_fap_tail's
  if (s_ok && tid == 0) sm->fap_done = 1;
  __syncthreads();
  small_snap(sm, t.snap, s_ok ? t.init : nullptr, t.seq);
}
// (DIRECT: the launch with no assembly before it, ds_reg_direct_body; a
// template argument of its own, so the other instantiations carry none of it;
// LINES: its chunk loader, CERT: no qualifier stream, reg_run)
template <int AGG, bool SPEC, bool DIRECT = false, bool LINES = false, bool CERT = false>
#ifndef UG_LDS_CAP
#define UG_LDS_CAP 40960u  // (build knob) LDS a k_ug_ds_reg block claims: 40 KB = 4 blocks a CU
#endif
#ifndef UG_WPE
#define UG_WPE 0  // (build knob) waves per SIMD the register allocation aims at, 0: the compiler's choice
#endif
__global__ void __launch_bounds__(256)
#if UG_WPE
__attribute__((amdgpu_waves_per_eu(UG_WPE, UG_WPE)))
#endif
k_ug_ds_reg(DecodeArgs a, SpanDsArgs g, const uint32_t* ncells,
                                                   const uint32_t* vlen, FapArgs fap, UgTail t) {
  extern __shared__ uint8_t s_pad[];
  if (threadIdx.x == 0 && a.n_kept == 0xFFFFFFFFu) s_pad[0] = 1;
  if (SPEC && !sld(&t.sm->ug_go)) {
    // (speculative, no group: every block leaves at once — no counter; the
    // sharded tail, which packs this rank's neutral share, runs in block 0)
    if (t.sharded && blockIdx.x == 0) ug_fap_tail_spec(fap, t);
    return;
  }
  if constexpr (DIRECT) {
    // (the body counts its block done itself: one barrier pair per 4 runs)
    if (ds_reg_direct_body<AGG, LINES, CERT>(a, ncells, vlen, fap, &t.sm->ug_done)) ug_fap_tail_direct(fap, t);
    return;
  }
  ds_reg_body<AGG, SPEC>(a, g, ncells, vlen, 0u, fap);
  __shared__ uint32_t s_last;
  __builtin_amdgcn_s_waitcnt(0);  // (this wave's atomics acknowledged)
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(&t.sm->ug_done, 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  // (two tails: the host-sized one is the code the unsharded C3* launch was
  // measured with — folding the speculative logic into it cost that launch
  // ~2.5 %, same box, through the whole kernel's code generation)
  if (SPEC) ug_fap_tail_spec(fap, t);
  else ug_fap_tail(fap, t);
}
