// k_desccert.hip — the kernel of tsdbhip_desc_certify: every row's qualifiers
// read once, to prove of each row what the streaming kernels otherwise prove
// on every call (k_ds_reg.hip reg_run's `stage`, k_lockstep, k_ug_dev).
//
// The statement (TSDBHIP_DESC_QUALS_PROVEN, tsdbhip.h), of a row of nc >= 2
// cells whose first two qualifiers, big-endian 16-bit words, are q0 and q1:
//   d = q1 - q0 is positive and a multiple of 16 (one flags nibble, a positive
//   step of whole seconds), q0 + (nc - 1) d <= 0xFFFF (no wrap: every delta at
//   most 4095), and qualifier c equals q0 + c d for every c < nc.
// A row of fewer than two cells is proven. A row whose qualifiers do not lie
// inside [0, qual_nbytes) at an even offset is unproven, and none of its bytes
// is read (k_pack_sizes' check).
//
// A wave takes rows g, g + G, ... of the launch's G waves, the row's two
// fields by scalar loads. A row streams as the other streaming kernels do: a
// wave instruction is 64 lanes x 16 B contiguous (512 cells, 1 KB), up to
// CERT_INSTR of them in flight (a 3600-cell row: all of it), at the row's own
// residue — any even offset, as k_pack_copy's "unaligned" loader. A lane whose
// piece starts at or past the row's end reads the piece that holds the row's
// last cell instead (at most 14 B past the row, inside the 64-byte slack), and
// an instruction whose whole range is past the end is skipped, a scalar
// branch. Nothing before the row's first byte is read. Each lane compares its
// 8 qualifiers with the expected ones two at a time (one xor a dword: no carry
// between the halves, neither sum exceeding 0xFFFF), cells past the end masked.
#pragma once
#include "dev_common.h"
#include "k_ds_chunks.hip"

namespace tsdb {

constexpr uint32_t CERT_THREADS = 256, CERT_WAVES = CERT_THREADS / WAVE;
constexpr uint32_t CERT_INSTR = 8;  // wave instructions of one row in flight: 4096 cells

struct CertArgs {
  uint64_t n_rows;
  const uint32_t* ncells;  // [n_rows]
  const uint64_t* qoff;    // [n_rows]
  const uint8_t* qual;
  uint64_t qn;                  // qual_nbytes
  unsigned long long* n_bad;    // += the rows that fail the statement
};

typedef uint32_t cert_vec_t __attribute__((ext_vector_type(4), aligned(2)));
typedef uint16_t cert_u16_t __attribute__((aligned(2)));

// true: the row of nc >= 2 cells at `row` fails the statement (wave-uniform)
DEVI bool cert_row_bad(const uint8_t* row, uint32_t nc, uint32_t lane) {
  const uint32_t q0 = ufl(__builtin_bswap16(*(const cert_u16_t*)row));
  const uint32_t q1 = ufl(__builtin_bswap16(*(const cert_u16_t*)(row + 2)));
  if (q1 <= q0) return true;
  const uint32_t d = q1 - q0;
  if ((d & 15u) != 0 || (uint64_t)q0 + (uint64_t)(nc - 1) * d > 0xFFFFull) return true;
  const uint32_t inc = d * 0x00020002u;
  // (d >= 16 and no wrap: nc <= 4096 = CERT_INSTR x 512 cells, the whole row in one round of loads)
  uint32_t miss = 0;
  cert_vec_t v[CERT_INSTR];
#pragma unroll
  for (uint32_t i = 0; i < CERT_INSTR; i++) {
    const uint32_t ci = DCH * i;  // the instruction's first cell: wave-uniform
    if (i > 0 && ci >= nc) continue;
    const uint32_t c = ci + 8u * lane;
    v[i] = *(const cert_vec_t*)(row + 2ull * (c < nc ? c : (nc - 1) & ~7u));
  }
#pragma unroll
  for (uint32_t i = 0; i < CERT_INSTR; i++) {
    const uint32_t ci = DCH * i;
    if (i > 0 && ci >= nc) continue;
    const uint32_t c = ci + 8u * lane;
    const uint32_t nmine = c < nc ? min(8u, nc - c) : 0u;
    uint32_t e = (q0 + c * d) * 0x00010001u + (d << 16);
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      uint32_t x = qpair(v[i][k]) ^ e;
      x &= nmine >= 2u * k + 2 ? 0xFFFFFFFFu : (nmine == 2u * k + 1 ? 0x0000FFFFu : 0u);
      miss |= x;
      e += inc;
    }
  }
  return ballot(miss != 0) != 0;
}

__global__ void __launch_bounds__(CERT_THREADS) k_desc_certify(CertArgs a) {
  const uint32_t lane = lane_id();
  const uint64_t g = (uint64_t)blockIdx.x * CERT_WAVES + ufl(threadIdx.x / WAVE);
  const uint64_t G = (uint64_t)gridDim.x * CERT_WAVES;
  uint32_t nbad = 0;
  for (uint64_t r = g; r < a.n_rows; r += G) {
    const uint32_t nc = sld(&a.ncells[r]);
    const uint64_t qo = sld(&a.qoff[r]);
    // (the row inside the buffer before any byte of it is read)
    if ((qo & 1) != 0 || qo > a.qn || 2ull * nc > a.qn - qo) {
      nbad++;
      continue;
    }
    if (nc >= 2 && cert_row_bad(a.qual + qo, nc, lane)) nbad++;
  }
  if (lane == 0 && nbad) atomicAdd(a.n_bad, (unsigned long long)nbad);
}

}  // namespace tsdb
