// k_scanrows.hip — kernels of tsdbhip_scan_rows: the rows of a resident table
// that the Scanner of TsdbQuery.getScanner delivers (TsdbQuery.java:368-394:
// the start / stop keys and the key regexp of createAndSetFilter, :433-492).
//
//   k_sr_match   a wave per 64 consecutive rows, the waves striding over the
//                table: fs_check_key (first offending row: one atomicMin word),
//                sr_match, and per row a selected flag and the selected key's
//                length. <false>: a lane byte-loads its own key, as k_fs_keys
//                does. <true>: the wave loads the contiguous keys of its 64 rows
//                in 16-byte pieces into its own LDS region and every lane reads
//                its key from there
//   (scans)      dscan_u64 over the flags and over the lengths
//   k_sr_emit    a lane per row: a selected row's index, key offset, key bytes
//                and gathered metadata at its scanned position
#pragma once
#include "dev_common.h"
#include "scanrows_host.h"

namespace tsdb {

constexpr uint32_t SR_THREADS = 256, SR_WAVES = SR_THREADS / WAVE;
constexpr uint32_t SR_BLOCKS = 2048;  // k_sr_match's grid at most: 8 blocks a CU
// A wave's LDS region: the keys of 64 rows, from the 16-byte line their first
// byte lies in. 4096 B hold 64 keys of up to 63 B (the 31-byte keys of the
// flood workload take 2 KB); the longest legal key is 8 + 4 + 8 * 16 = 140 B,
// and a wave whose 64 keys need more than the region byte-loads them instead.
// 16 KB a block: 8 blocks a CU fit the 160 KB.
constexpr uint32_t SR_REGION = 4096;

struct SrMatchArgs {
  FsRows in;
  SrQuery q;
  unsigned long long* err;
  uint64_t* flags;  // [n] 1: selected
  uint64_t* klen;   // [n] a selected row's key length, else 0
};

template <bool LDS>
__global__ void __launch_bounds__(SR_THREADS) k_sr_match(SrMatchArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_keys[LDS ? SR_WAVES * SR_REGION : 16];
  const uint32_t lane = lane_id(), wave = threadIdx.x / WAVE;
  const uint64_t gwave = (uint64_t)blockIdx.x * SR_WAVES + wave, nwaves = (uint64_t)gridDim.x * SR_WAVES;
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.in.key_off[a.in.n] != a.in.key_nbytes)
    atomicMin(a.err, (unsigned long long)FS_E_END);
  for (uint64_t r0 = gwave * WAVE; r0 < a.in.n; r0 += nwaves * WAVE) {
    const uint64_t r64 = r0 + lane;
    const bool active = r64 < a.in.n;
    const uint32_t r = (uint32_t)r64;
    uint64_t o0 = 0, o1 = 0;
    uint32_t cls = 0;
    if (active) {
      o0 = a.in.key_off[r];
      o1 = a.in.key_off[r + 1];
      cls = fs_check_key(a.in, o0, o1);
    }
    const uint32_t len = (uint32_t)(o1 - o0);  // (cls == 0: at most 140)
    bool sel = false;
    bool from_lds = false;
    if (LDS) {
      // Every active lane's o0 <= o1 <= key_nbytes, and lane l's o1 is lane
      // l + 1's o0 (the same word): the 65 offsets are monotone and inside
      // key_nbytes, the wave's keys are key[lo, hi).
      const bool offs_ok = __ballot(active && cls == FS_E_OFF) == 0;
      const uint32_t n_act = (uint32_t)__popcll(__ballot(active));
      const uint64_t lo = __shfl(o0, 0), hi = __shfl(o1, (int)n_act - 1);
      const uint8_t* base = a.in.key + lo;
      const uint32_t d = (uint32_t)((uintptr_t)base & 15u);  // the first piece is aligned down
      const uint64_t span = hi - lo + d;
      uint8_t* reg = s_keys + wave * SR_REGION;
      if (offs_ok && span <= SR_REGION) {
        from_lds = true;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();  // (the previous round's reads are done)
        const uint32_t pieces = ((uint32_t)span + 15u) / 16u;
        for (uint32_t p = lane; p < pieces; p += WAVE) {
          // piece p: image bytes [16 p, 16 p + 16), key bytes from lo - d + 16 p
          const uint32_t i0 = 16u * p;
          // whole if it lies inside key[0, key_nbytes) (the bytes before lo and from hi on are other rows' keys)
          if ((i0 >= d || lo >= d) && lo - d + i0 + 16u <= a.in.key_nbytes) {
            *(uint4*)(reg + i0) = *(const uint4*)(base - d + i0);
          } else {  // the table's first and last piece: byte by byte, only the wave's own bytes
            const uint32_t b0 = i0 < d ? d : i0, b1 = i0 + 16u < (uint32_t)span ? i0 + 16u : (uint32_t)span;
            for (uint32_t b = b0; b < b1; b++) reg[b] = base[b - d];
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (active && cls == 0) sel = sr_match((const uint8_t*)reg + (uint32_t)(o0 - lo) + d, len, a.in, a.q);
      }
    }
    if (!from_lds && active && cls == 0) sel = sr_match(a.in.key + o0, len, a.in, a.q);
    if (active) {
      if (cls) atomicMin(a.err, ((unsigned long long)r << 8) | cls);
      a.flags[r] = sel ? 1ull : 0ull;
      a.klen[r] = sel ? (uint64_t)len : 0ull;
    }
  }
}

struct SrEmitArgs {
  uint32_t n;
  bool cells;
  const uint64_t* key_off;
  const uint8_t* key;
  const uint8_t* status;  // null: none to gather
  const uint64_t* in_qoff;
  const uint32_t* in_qlen;
  const uint64_t* in_voff;
  const uint32_t* in_vlen;
  const uint64_t* flags;
  const uint64_t* fscan;   // rows selected before r
  const uint64_t* kscan;   // their key bytes
  const uint64_t* totals;  // [0] rows selected, [1] key bytes
  uint32_t* row_index;
  uint64_t* out_key_off;
  uint8_t* out_key;
  uint8_t* out_status;
  uint64_t* out_qoff;
  uint32_t* out_qlen;
  uint64_t* out_voff;
  uint32_t* out_vlen;
};

// (launched after the host has checked the totals against the capacities: an
// output row < n_selected <= row_capacity, a key ends at or before key_used <=
// key_capacity)
__global__ void __launch_bounds__(256) k_sr_emit(SrEmitArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0) a.out_key_off[a.totals[0]] = a.totals[1];
  if (r >= a.n || !a.flags[r]) return;
  const uint64_t p = a.fscan[r], ko = a.kscan[r], o0 = a.key_off[r], len = a.key_off[r + 1] - o0;
  a.row_index[p] = r;
  a.out_key_off[p] = ko;
  for (uint64_t b = 0; b < len; b++) a.out_key[ko + b] = a.key[o0 + b];
  if (a.status) a.out_status[p] = a.status[r];
  if (a.cells) {
    a.out_qoff[p] = a.in_qoff[r];
    a.out_qlen[p] = a.in_qlen[r];
    a.out_voff[p] = a.in_voff[r];
    a.out_vlen[p] = a.in_vlen[r];
  }
}

}  // namespace tsdb
