/*
 * tsdbhip.h — C-ABI of libtsdbhip.so, the MI355X (gfx950) query-time
 * aggregation path of OpenTSDB 1.1 (reference: anonthing/opentsdb).
 *
 * Plain pointers and sizes only; no HIP, torch or C++ types cross this
 * boundary, so the Java host binds it through a thin JNI shim (see
 * INTEGRATION.md) and Python through ctypes (opentsdb_amd/_lib.py).
 *
 * What each entry point replaces in the reference (paths relative to the
 * reference root):
 *
 *   tsdbhip_spangroup_run  — the whole lazy iteration of a SpanGroup as the
 *       consumers drive it (GraphHandler.java:791-808, Plot.java:190-204,
 *       CliQuery.java:161-170): SpanGroup ctor/add (SpanGroup.java:104-142),
 *       SGIterator (SpanGroup.java:370-796), Span.Iterator /
 *       Span.DownsamplingIterator (Span.java:248-530), RowSeq.Iterator
 *       (RowSeq.java:360-497) and the five Aggregators (Aggregators.java:76-243).
 *       Row assembly follows Span.addRow / RowSeq.addRow (Span.java:87-132,
 *       RowSeq.java:92-172), i.e. what TsdbQuery.findSpans does with each
 *       compacted KeyValue (TsdbQuery.java:240-285).
 *   tsdbhip_spangroup_run_batch — the SpanGroup[] of a GROUP BY query
 *       (TsdbQuery.groupByAndAggregate, TsdbQuery.java:294-363), all groups in
 *       one call.
 *   tsdbhip_groupby_plan — the grouping loop of TsdbQuery.groupByAndAggregate
 *       itself (TsdbQuery.java:310-348: Tags.getValueId per GROUP BY tag,
 *       Tags.java:213-227, the ByteMap of group keys, the dropped spans of
 *       :339-344) and SpanGroup.getTags / getAggregatedTags of every group
 *       (computeTags, SpanGroup.java:149-191), from the spans' row keys.
 *   tsdbhip_scan_rows — the Scanner of TsdbQuery.getScanner (TsdbQuery.java:
 *       368-492: start / stop keys and createAndSetFilter's key regexp) over a
 *       table of row keys, host or device resident.
 *   tsdbhip_find_spans — the TreeMap under SpanCmp that TsdbQuery.findSpans
 *       fills from the scanned rows (TsdbQuery.java:240-285, 594-621).
 *   tsdbhip_desc_gather — the repacking of the spans' rows into the plan's
 *       batch order for a descriptor already in HBM.
 *   tsdbhip_desc_pack — the bridge's copy of each compacted KeyValue to aligned
 *       offsets (TsdbQuery.java:264-266 as packing.pack_spans does it) for a
 *       descriptor already in HBM.
 *   tsdbhip_desc_certify — no counterpart: the proof, made once for a resident
 *       table, that every row's qualifiers are regular (the streaming kernels
 *       then read the values alone).
 *   tsdbhip_format_points — the text GraphHandler.respondAsciiQuery,
 *       Plot.dumpToFiles and CliQuery print for each DataPoint.
 *   tsdbhip_compact_rows   — CompactionQueue.compact(row, compacted[])
 *       (CompactionQueue.java:243-435, 450-743) for a batch of rows.
 *   tsdbhip_host_register / unregister — pinning of the JNI DirectByteBuffers
 *       the bridge packs at TsdbQuery.java:264-266.
 *
 * Errors map to the reference's exceptions (the JNI shim rethrows them):
 *   TSDBHIP_E_ILLEGAL_DATA -> IllegalDataException   (RowSeq.java:203,223;
 *                             CompactionQueue.java:324,538,640,717,736)
 *   TSDBHIP_E_NAN_INF      -> IllegalStateException  (SpanGroup.java:660-663)
 *   TSDBHIP_E_EMPTY_SPAN   -> AssertionError         (SpanGroup.java:452-455)
 *   others                 -> RuntimeException
 * The reference is lazy (exceptions surface while iterating); this library
 * is eager. out->err_index carries the index of the first output point the
 * reference would NOT have delivered (-1 when unknown), so a host adapter can
 * replay the lazy behaviour.
 */
#ifndef TSDBHIP_H
#define TSDBHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSDBHIP_ABI_VERSION 8

/* ---- return codes ---------------------------------------------------- */
#define TSDBHIP_OK               0
#define TSDBHIP_E_ILLEGAL_DATA  -1
#define TSDBHIP_E_NAN_INF       -2
#define TSDBHIP_E_EMPTY_SPAN    -3
#define TSDBHIP_E_CAPACITY      -4
#define TSDBHIP_E_HIP           -5
#define TSDBHIP_E_RCCL          -6
#define TSDBHIP_E_INVALID_ARG   -7
#define TSDBHIP_E_UNSORTED      -8  /* cells of a span not strictly increasing
                                       after row assembly: input the reference
                                       never produces from compacted rows */
#define TSDBHIP_E_OUT_OF_BOUNDS -9  /* reference would throw
                                       ArrayIndexOutOfBoundsException */
#define TSDBHIP_E_NO_DEVICE    -10
#define TSDBHIP_E_UNSUPPORTED  -11 /* reserved (ABI v2 raised it for a Q1
                                       seek whose shifted reads cross merged
                                       rows; v3 reproduces those reads)      */

/* ---- aggregator op codes (Aggregators.java:44-48 names) --------------- */
#define TSDBHIP_AGG_SUM 0
#define TSDBHIP_AGG_MIN 1
#define TSDBHIP_AGG_MAX 2
#define TSDBHIP_AGG_AVG 3
#define TSDBHIP_AGG_DEV 4

/* tsdbhip_timing.hot_kernel */
#define TSDBHIP_HOT_NONE        0
#define TSDBHIP_HOT_DS_CHUNKS   1 /* k_ds_reg (+ k_ds_spans): streaming decode+downsample */
#define TSDBHIP_HOT_DECODE_FAST 2 /* streaming per-span decode(+downsample) */
#define TSDBHIP_HOT_DECODE_GEN  3 /* general per-span decode(+downsample)   */
#define TSDBHIP_HOT_REDUCE_DIRECT 5 /* k_reduce over direct spans (no-downsampling path) */
#define TSDBHIP_HOT_LOCKSTEP    6 /* k_lockstep: one pass over qualifiers + values of a lockstep group */
#define TSDBHIP_HOT_UG_DS_REG   7 /* k_ug_ds_reg: the uniform aligned group in one launch */
#define TSDBHIP_HOT_UG_DEV      8 /* k_ug_dev: integer dev chains of a uniform group */
#define TSDBHIP_HOT_DS_E        9 /* k_ds_reg in the uniform E variant: the spans' bucket values
                                     on the key's buckets (k_ug_reduce runs after it) */
#define TSDBHIP_HOT_GROUPBY    10 /* k_gb_count + scan + k_gb_scatter: the radix sort passes of
                                     tsdbhip_groupby_plan */
#define TSDBHIP_HOT_FIND_SPANS 11 /* k_gb_count + scan + k_gb_scatter over the rows' live key
                                     digits: the sort passes of tsdbhip_find_spans */
#define TSDBHIP_HOT_COMPACT     4 /* k_compact_wave: every row's classification and compaction
                                     in one pass (tsdbhip_compact_rows)      */

/* ---- desc flags ------------------------------------------------------- */
#define TSDBHIP_DESC_DEVICE   0x1u /* every array pointer in the desc is a
                                      device pointer (data already in HBM) */
#define TSDBHIP_EXACT_ORDER   0x2u /* reduce over spans strictly in span order
                                      (bit-exact double sums / dev; slower) */
#define TSDBHIP_SHARDED       0x4u /* desc holds this rank's shard of the
                                      group; exchange with the other ranks of
                                      the communicator set by tsdbhip_comm_init */
#define TSDBHIP_DESC_QUALS_PROVEN 0x8u /* (with TSDBHIP_DESC_DEVICE) the rows'
                                      qualifiers were proven regular and have
                                      not changed since: tsdbhip_desc_certify */

typedef struct tsdbhip_ctx tsdbhip_ctx;

/*
 * One SpanGroup: the spans (in TreeMap order, TsdbQuery.java:242-243) and
 * the compacted KeyValues of each span, rows sorted by time within a span.
 * qual_bytes / val_bytes hold exactly the KeyValue qualifier()/value() bytes
 * (big-endian, as stored in HBase); a row's qualifier offset must be even.
 *
 * Layout (tests/layouts.py, tests/test_layouts.py: every kernel path on each
 * of these). Rows may lie anywhere inside qual_bytes / val_bytes, in any order
 * (offsets need not grow with the row index: tsdbhip_desc_gather's output,
 * a shuffled or reversed buffer) and at any value offset; qualifier offsets
 * must be even; rows must not share bytes. Bytes outside rows (a lead, gaps,
 * the tail; tsdbhip_rows_out's "bytes between rows") are read by the wide
 * loads and never interpreted: results do not depend on them. What keeps a
 * row on the streaming paths is its alignment, 8 B for its qualifier offset
 * and 16 B for its value offset (packing.pack_spans' layout); the lockstep /
 * uniform paths without downsampling (k_lockstep, k_ug_dev) take any even
 * qualifier offset with a value offset that is a multiple of the cell width.
 * Any other row takes the general path at its cost, and a group that holds
 * one falls back as a whole from the aligned group and its direct form
 * (tsdbhip_timing.paths: TSDBHIP_PATH_ALIGNED_RERUN, _UNIFORM_FALLBACK,
 * _GROUP_DIRECT_FALLBACK): tsdbhip_compact_rows' placement (value offsets at
 * every residue) is such a layout.
 * With TSDBHIP_DESC_DEVICE the allocations behind qual_bytes and val_bytes
 * must be readable for 64 bytes past qual_nbytes / val_nbytes (their
 * contents are never interpreted): the loaders read whole groups past a
 * row's end, at most k_ds_chunks.hip load_raw's 7 cells (56 B of values, 14 B
 * of qualifiers; k_decode_fast.hip load_chunk 3 cells; k_lockstep.hip and
 * k_ds_reg.hip reg_run a 16-B group, 14 B), and dev_common.h load_be_bytes
 * 12 B from the dword that holds a value's first byte. A host descriptor
 * needs no such slack: its buffers are copied with it added.
 *
 * Timestamps are 32 bits: the one deliberate departure from the reference.
 * A row key holds 4 bytes of base time and a qualifier up to 4095 s on top of
 * it, so a cell of the last hourly row (base 4294965600) can lie at or beyond
 * 2^32. The reference carries such a timestamp as a long: alone in its group
 * the cell is emitted when end_time admits it, and next to a second span the
 * interpolation towards it throws (SpanGroup.java:719-727, "x1 out of
 * range"). Here a span with a cell at or beyond 2^32 fails the call with
 * TSDBHIP_E_INVALID_ARG (err_index 0, nothing emitted) while the spans are
 * assembled, before any kernel runs on its cells and whatever the window.
 * An end_time above 2^32 - 1 is therefore equivalent to 2^32 - 1, and a
 * start_time above it keeps no span. Every cell of a row counts, whatever
 * the order of the row's cells (a row with cells out of order that all lie
 * below 2^32 is TSDBHIP_E_UNSORTED, as before).
 *
 * A span whose first cell is at timestamp 0 fails the call with
 * TSDBHIP_E_OUT_OF_BOUNDS (err_index 0), as the reference does: Span.addRow
 * starts from last_ts = 0, takes such a first row for one added out of order
 * (Span.java:126) and throws from the log message's rows.get(rows.size() - 1)
 * on the empty list, while TsdbQuery.findSpans scans the rows.
 */
typedef struct tsdbhip_sg_desc {
  int64_t  start_time;      /* SpanGroup start (u32 held in int64)        */
  int64_t  end_time;        /* SpanGroup end   (u32 held in int64)        */
  uint8_t  rate;            /* SpanGroup.rate                              */
  uint8_t  agg;             /* TSDBHIP_AGG_*  cross-series aggregator      */
  uint8_t  ds_agg;          /* TSDBHIP_AGG_*  downsampler (ds_interval>0)  */
  uint8_t  reserved0;
  uint32_t flags;           /* TSDBHIP_DESC_DEVICE | TSDBHIP_EXACT_ORDER.. */
  int32_t  ds_interval;     /* seconds, 0 = no downsampling                */
  uint32_t n_spans;
  uint64_t n_rows;
  const uint64_t* span_row_start; /* [n_spans+1] rows of span s are
                                     [span_row_start[s], span_row_start[s+1]) */
  const uint32_t* row_base;       /* [n_rows] base_time from the row key      */
  const uint32_t* row_ncells;     /* [n_rows] qualifier().length / 2          */
  const uint64_t* row_qual_off;   /* [n_rows] byte offset into qual_bytes     */
  const uint64_t* row_val_off;    /* [n_rows] byte offset into val_bytes      */
  const uint32_t* row_val_len;    /* [n_rows] value().length                  */
  const uint8_t*  qual_bytes;
  uint64_t        qual_nbytes;
  const uint8_t*  val_bytes;
  uint64_t        val_nbytes;
  uint64_t        span0;    /* TSDBHIP_SHARDED: global index (TreeMap order)
                               of this shard's first span; the ranks agree on
                               the error the reference throws first by global
                               span order (ABI v4). 0 otherwise.           */
} tsdbhip_sg_desc;

/* Result of one SpanGroup, in emission order (SGIterator order). */
typedef struct tsdbhip_sg_out {
  uint64_t capacity;        /* in:  size of ts/is_int/bits                 */
  int64_t* ts;              /* out: DataPoint.timestamp()                  */
  uint8_t* is_int;          /* out: DataPoint.isInteger()                  */
  int64_t* bits;            /* out: longValue() or doubleToRawLongBits()   */
  uint64_t n_out;           /* out: SpanGroup.size()                       */
  uint64_t n_input_points;  /* out: SpanGroup.aggregatedSize()             */
  int32_t  err_code;        /* out: same as the return code                */
  int32_t  reserved0;
  int64_t  err_index;       /* out: first output index not delivered by the
                               lazy reference, or -1 if unknown / no error  */
} tsdbhip_sg_out;

/* Per-call device timings of the last tsdbhip_spangroup_run on a ctx,
 * measured with HIP events on the ctx stream (milliseconds). After
 * tsdbhip_compact_rows: total_ms (the call), and under "timing_detail"
 * hot_ms = k_compact_wave, grid_ms = k_compact_rows, reduce_ms =
 * k_compact_complex + k_compact_dups; hot_kernel = TSDBHIP_HOT_COMPACT. */
typedef struct tsdbhip_timing {
  float    total_ms;        /* first kernel start .. last kernel end        */
  float    decode_ms;       /* decode(+downsample) kernel — dominant, HBM   */
  float    grid_ms;         /* union-grid construction                      */
  float    reduce_ms;       /* cross-span reduction + combine               */
  float    exchange_ms;     /* RCCL exchange (sharded runs, "timing_detail") */
  float    hot_ms;          /* the dominant HBM-streaming kernel alone      */
  uint32_t hot_kernel;      /* TSDBHIP_HOT_*: which kernel hot_ms timed      */
  uint32_t n_collectives;   /* sharded calls: collective launches this rank
                               issued (one per RCCL group)                  */
  uint64_t decode_bytes;    /* algorithmic bytes read+written by decode      */
  uint64_t alg_bytes;       /* SURVEY §8(d) algorithmic bytes of the call   */
  uint64_t n_grid;          /* |G|                                           */
  uint64_t n_emitted;       /* Σ|E_s| (points after downsampling)           */
  uint32_t paths;           /* TSDBHIP_PATH_* bits: which variants ran (ABI v5) */
  uint32_t late_stamp;      /* 1: the call-end stamp (the host's proof that the
                               snapshot and results are this call's) arrived
                               only after the stream sync; summed in totals */
  uint64_t x_bytes;         /* sharded calls: bytes this rank received in the
                               call's collectives (ABI v6)                  */
  uint64_t h2d_bytes;       /* bytes of host-resident inputs the call copied
                               to HBM (a rerun copies none again; ABI v7)  */
} tsdbhip_timing;
/* tsdbhip_timing.paths */
#define TSDBHIP_PATH_ALIGNED_GROUP 1u  /* k_ds_reg's aligned-group reduction
                                          stood for E + the reduce            */
#define TSDBHIP_PATH_ALIGNED_RERUN 2u  /* it was tried, a span fell outside the
                                          group: E rewritten, usual reduce    */
#define TSDBHIP_PATH_LOCKSTEP      4u  /* no downsampling, every span on one
                                          cadence: k_lockstep's single pass   */
#define TSDBHIP_PATH_DIRECT_REDO   8u  /* k_lockstep found a qualifier off the
                                          proposal: the call ran again on the
                                          proven (scan + reduce) path         */
#define TSDBHIP_PATH_UNIFORM      16u  /* every kept span proposed one class key
                                          at assembly: G from the key, no grid
                                          kernels, one host round trip        */
#define TSDBHIP_PATH_UNIFORM_FALLBACK 32u  /* the uniform aligned group did not
                                          stand: the general path ran the call */
#define TSDBHIP_PATH_GROUP_DIRECT 64u  /* the aligned group of one-row spans ran
                                          straight from the descriptor: no
                                          assembly, no kept list, no host round
                                          trip before the streaming kernel    */
#define TSDBHIP_PATH_GROUP_DIRECT_FALLBACK 128u  /* it was tried and the group
                                          did not stand: the call ran again
                                          from assembly                       */
#define TSDBHIP_PATH_GROUP_DIRECT_LINES 256u  /* that launch (taken or fallen
                                          back) read the values in whole lines
                                          ("group_direct_load" lines_nt)      */
#define TSDBHIP_PATH_QUALS_PROVEN 512u  /* that launch (taken or fallen back)
                                          ran without the qualifier stream: the
                                          descriptor carried
                                          TSDBHIP_DESC_QUALS_PROVEN             */

/* ---- row compaction (CompactionQueue.compact) -------------------------- */
/*
 * A batch of HBase rows, each a list of KeyValues (qualifier, value) in the
 * order HBase returns them (sorted by qualifier bytes). For every row the
 * library computes compacted[0] of CompactionQueue.compact(row, compacted)
 * (CompactionQueue.java:243-435) — the cell TsdbQuery.findSpans hands to
 * Span.addRow (TsdbQuery.java:264-266).
 *
 * Layout (chosen so the per-KV metadata stays small next to the ~7 bytes of
 * cell data per KV): the qualifiers of row r's KVs are packed back to back,
 * in KV order, in qual_bytes[row_qual_off[r], row_qual_off[r+1]); likewise
 * the values in val_bytes[row_val_off[r], row_val_off[r+1]). Per KV only the
 * two lengths are passed (u16: an OpenTSDB qualifier is at most 2*4096 bytes
 * and a compacted value at most 8*4096+1). Offsets must be non-decreasing
 * and each row's lengths must add up to its extents, else
 * TSDBHIP_E_INVALID_ARG.
 */
typedef struct tsdbhip_rows_desc {
  uint32_t flags;               /* TSDBHIP_DESC_DEVICE: desc AND out arrays
                                   are device pointers                      */
  uint32_t reserved0;
  uint64_t n_rows;
  uint64_t n_kvs;
  const uint64_t* row_kv_start; /* [n_rows+1] KVs of row r                   */
  const uint64_t* row_qual_off; /* [n_rows+1] qualifier bytes of row r       */
  const uint64_t* row_val_off;  /* [n_rows+1] value bytes of row r           */
  const uint16_t* kv_qual_len;  /* [n_kvs] qualifier().length                */
  const uint16_t* kv_val_len;   /* [n_kvs] value().length                    */
  const uint8_t*  qual_bytes;
  uint64_t        qual_nbytes;
  const uint8_t*  val_bytes;
  uint64_t        val_nbytes;
} tsdbhip_rows_desc;

/* Row status codes for tsdbhip_rows_out.row_status */
#define TSDBHIP_ROW_NONE     0  /* compacted[0] stays null (empty / junk)     */
#define TSDBHIP_ROW_SINGLE   1  /* the single KV, possibly float-fixed        */
#define TSDBHIP_ROW_TRIVIAL  2  /* trivialCompact                             */
#define TSDBHIP_ROW_COMPLEX  3  /* complexCompact                             */
#define TSDBHIP_ROW_ERROR    4  /* IllegalDataException                       */
#define TSDBHIP_ROW_OOB      5  /* ArrayIndexOutOfBoundsException
                                   (breakDownValues on a malformed compacted
                                   cell, CompactionQueue.java:708,722)       */

/*
 * Output: row r's compacted qualifier is written at
 *   qual_bytes[row_qual_off[r] - row_qual_off[0]]   (never longer than the
 *   row's input qualifiers), its value at
 *   val_bytes[row_val_off[r] - row_val_off[0] + r]  (never longer than the
 *   row's input values + 1 meta byte),
 * so one pass needs no output scan: qual_capacity >= qualifier extent and
 * val_capacity >= value extent + n_rows. Bytes between rows are undefined.
 * Rows with status NONE/ERROR/OOB have length 0.
 */
typedef struct tsdbhip_rows_out {
  uint64_t qual_capacity;    /* in: bytes available in qual_bytes           */
  uint64_t val_capacity;     /* in: bytes available in val_bytes            */
  uint8_t*  row_status;      /* [n_rows]                                     */
  uint64_t* row_qual_off;    /* [n_rows] offset of the compacted qualifier   */
  uint32_t* row_qual_len;    /* [n_rows]                                     */
  uint64_t* row_val_off;     /* [n_rows]                                     */
  uint32_t* row_val_len;     /* [n_rows]                                     */
  uint8_t*  qual_bytes;      /* out                                          */
  uint8_t*  val_bytes;       /* out                                          */
  uint64_t  qual_used;       /* out: qualifier extent written               */
  uint64_t  val_used;        /* out: value extent written                   */
  uint64_t  n_complex;       /* out: rows that reached complexCompact
                                (status COMPLEX, ERROR or OOB)             */
  /* The write/delete decision of compact() (CompactionQueue.java:276,
   * 355-404, 419-434) for a row whose base time is old enough to be written
   * back (the caller applies the cut-off of :408-413 and
   * TSDB.enable_compactions). Both arrays are optional (NULL: not produced).
   *   row_write[r]   1: tsdb.put(key, compacted qualifier, compacted value)
   *                  (TRIVIAL rows, and COMPLEX rows unless a KV of the row
   *                  already holds exactly the compacted qualifier AND
   *                  value, :388-396); 0 otherwise.
   *   row_keep_kv[r] index, relative to row_kv_start[r], of the KV that
   *                  holds the compacted qualifier (:364-400) and must NOT
   *                  be deleted; -1 if none.
   * The delete set of a TRIVIAL/COMPLEX row (tsdb.delete, :421-434) is every
   * KV of the row whose qualifier length is even and non-zero (junk KVs were
   * dropped from the list, :301-306), except row_keep_kv. SINGLE / NONE /
   * ERROR / OOB rows: no put, no delete (:245-269 return before any write;
   * an exception aborts the row). */
  uint8_t*  row_write;       /* [n_rows] or NULL                             */
  int32_t*  row_keep_kv;     /* [n_rows] or NULL                             */
} tsdbhip_rows_out;

/* ---- synthetic, HBM-resident inputs (bench / tests) -------------------- */
#define TSDBHIP_SYN_INT64_COUNTER 0 /* 8-byte longs (flags 0x7), monotone
                                       counter, increments in (0,1000)       */
#define TSDBHIP_SYN_FLOAT32       1 /* 4-byte floats (flags 0xB), ~100+N(0,1) */
#define TSDBHIP_SYN_FLOAT64       2 /* 8-byte doubles (flags 0xF)             */

typedef struct tsdbhip_synth_params {
  uint64_t seed;
  uint32_t n_spans;
  uint32_t n_points;        /* points per span                              */
  uint32_t t0;              /* first timestamp (divisible by 3600)          */
  uint32_t step;            /* cadence in seconds (divides 3600)            */
  uint32_t kind;            /* TSDBHIP_SYN_*                                */
  uint32_t span0;           /* global index of the first span (shards)      */
} tsdbhip_synth_params;

/* ---- context ----------------------------------------------------------- */
/*
 * A context owns a pool of per-call slots (HIP stream, HBM scratch, pinned
 * staging): every entry point is re-entrant, and calls from several host
 * threads on one context run concurrently, each on its own slot (the
 * reference's Netty workers and gnuplot pool threads call SpanGroup
 * concurrently, GraphHandler.java:182,285). tsdbhip_last_error is the calling
 * thread's last message; tsdbhip_last_timing the calling thread's last call
 * on that context.
 */
int         tsdbhip_open(int32_t device, tsdbhip_ctx** out);
/*
 * One context over several GPUs of this process (the JVM's, TsdbQuery.java:
 * 301-307): tsdbhip_spangroup_run splits each SpanGroup into contiguous span
 * ranges (span order kept, balanced by points for host descs), runs rank r on
 * devices[r] from a host thread of its own, and exchanges grid and partials
 * over RCCL (ncclCommInitAll) when the devices are distinct; when a device
 * repeats, the ranks sharing it exchange through device copies (several
 * shards on one GPU: same results, used to run the N-rank exchange on one
 * GPU). tsdbhip_open_mask: the devices of the set bits of gpu_mask.
 * Compaction, group-by batches, synthetic inputs and probes of a
 * multi-device context run on its first device. */
int         tsdbhip_open_devices(const int32_t* devices, uint32_t n, tsdbhip_ctx** out);
/* Path / diagnostic options of a context and of its member contexts (ABI v6;
 * results never depend on them: the tests use them to run every kernel
 * variant, A/B runs to compare; no environment variable is read):
 *   "decode"        "auto" | "general" | "fast" | "chunks" | "spans" | "direct"
 *   "aligned_group" "on" | "off"   k_ds_reg's aligned-group reduction
 *   "lockstep"      "on" | "off" | "always"   the lockstep proposal (k_lockstep):
 *                   "on" for groups of >= 2048 lockstep waves (and sharded
 *                   groups), "always" for any group
 *   "group_direct"  "on" | "off" | "always"   the aligned group of one-row spans
 *                   launched with no assembly before it (as many rows as spans,
 *                   an aligned-group query): "on" for groups of more than 4096
 *                   spans, "always" for any group; a group that is not one runs
 *                   again from assembly (TSDBHIP_PATH_GROUP_DIRECT*)
 *   "group_direct_run" "auto" | "fill" | "1" | "2" | "4" | ... | "256"   spans a
 *                   wave of that launch streams as one run (wave g of G: spans
 *                   g, g + G, ...): a number r gives ceil(n / 4 r) blocks;
 *                   "fill" gives min(ceil(n / 4), resident blocks), one
 *                   generation of blocks whose waves share the whole group;
 *                   "auto": "fill"
 *   "group_direct_blocks" "auto" | a positive count   what "fill" takes for the
 *                   resident blocks: "auto" the device's (CUs x the blocks a CU
 *                   holds of that kernel); a count lets a small group reach
 *                   long runs (tests)
 *   "group_direct_load" "auto" | "rows" | "lines_nt"   how that launch loads a
 *                   chunk's values: "rows", a lane its own 8 cells (lanes 64 B
 *                   apart); "lines_nt", a wave instruction 1 KB contiguous with
 *                   non-temporal loads, transposed through LDS; "auto":
 *                   "lines_nt" (TSDBHIP_PATH_GROUP_DIRECT_LINES)
 *   "quals_proven"  "auto" | "off" | "rank0"   "auto": that launch does not read
 *                   the qualifiers of a device descriptor that carries
 *                   TSDBHIP_DESC_QUALS_PROVEN (TSDBHIP_PATH_QUALS_PROVEN); "off":
 *                   it reads and proves them on every call whatever the flag;
 *                   "rank0": "auto" on rank 0 of a sharded call and "off" on
 *                   every other rank (tests: the ranks of a multi-device
 *                   context share one descriptor). Results never depend on it
 *   "scan_rows_load" "auto" | "lanes" | "lds"   how tsdbhip_scan_rows' match
 *                   kernel reads the keys: "lanes", a lane its own key byte by
 *                   byte; "lds", a wave the keys of its 64 rows in 16-byte
 *                   pieces through LDS; "auto": "lds" 
 *   "scan_rows_blocks" "auto" | a positive count   that kernel's grid at most
 *                   (its waves stride over the table; a count lets a small
 *                   table reach the second round: tests)
 *   "desc_pack_load" "auto" | "unaligned" | "shift"   how tsdbhip_desc_pack's copy
 *                   kernel loads a row's bytes: "unaligned", one load of the
 *                   store's width at the row's own residue; "shift", dword-aligned
 *                   loads and v_alignbyte_b32; "auto": "unaligned" 
 *   "timing_detail" "on" | "off"   decode / grid event pairs in tsdbhip_timing
 *   "check_clean"   "on" | "off"   check the zero-on-entry invariants (stderr)
 *   "events"        "kernel" | "marker" | "none"   how tsdbhip_timing is measured:
 *                   HIP events carried by the kernel launches (default), event
 *                   markers between kernels (each can idle the GPU a few us),
 *                   or not at all (timings 0)
 * Unknown names or values: TSDBHIP_E_INVALID_ARG. */
int         tsdbhip_set_option(tsdbhip_ctx* ctx, const char* name, const char* value);
int         tsdbhip_open_mask(uint32_t gpu_mask, tsdbhip_ctx** out);
int         tsdbhip_ranks(tsdbhip_ctx* ctx);  /* shards per SpanGroup (1: one device) */
void        tsdbhip_close(tsdbhip_ctx* ctx);
const char* tsdbhip_last_error(tsdbhip_ctx* ctx);
int         tsdbhip_abi_version(void);

int tsdbhip_host_register(tsdbhip_ctx* ctx, void* p, size_t n);
int tsdbhip_host_unregister(tsdbhip_ctx* ctx, void* p);

/* ---- the hot path ------------------------------------------------------ */
int tsdbhip_spangroup_run(tsdbhip_ctx* ctx, const tsdbhip_sg_desc* desc,
                          tsdbhip_sg_out* out);
int tsdbhip_last_timing(tsdbhip_ctx* ctx, tsdbhip_timing* t);
/* Sums of the float timing fields (and of n_grid / n_emitted) over every
 * call on ctx since the last reset, and their count: a caller times many
 * calls without a per-call readout. reset != 0 zeroes them after reading. */
int tsdbhip_timing_totals(tsdbhip_ctx* ctx, tsdbhip_timing* sum, uint64_t* n_calls, int32_t reset);

/* ---- group-by batching ------------------------------------------------- */
/*
 * Every SpanGroup of one query's GROUP BY in one call — the array
 * TsdbQuery.groupByAndAggregate returns (TsdbQuery.java:294-363): the groups
 * share start/end/rate/aggregator/downsampler (one SpanGroup ctor call per
 * group with the query's arguments, TsdbQuery.java:346-348). `desc` holds the
 * spans of all groups, group g's spans being [group_span_start[g],
 * group_span_start[g+1]) in TreeMap order within the group, groups in the
 * ByteMap order of their tag-value keys; group_span_start is a host array of
 * n_groups+1 entries with [0] = 0 and [n_groups] = desc->n_spans. outs[g]
 * receives group g's points exactly as tsdbhip_spangroup_run on that group
 * alone would (same err_code / err_index per group). Returns TSDBHIP_OK, or
 * the first failing group's code (every outs[g].err_code is set). Not with
 * TSDBHIP_SHARDED. Per-call timings: tsdbhip_last_timing.
 */
int tsdbhip_spangroup_run_batch(tsdbhip_ctx* ctx, const tsdbhip_sg_desc* desc, uint32_t n_groups,
                                const uint32_t* group_span_start, tsdbhip_sg_out* outs);

/* ---- GROUP BY planning and SpanGroup tags (ABI v8) ---------------------- */
/*
 * tsdbhip_groupby_plan: the grouping of TsdbQuery.groupByAndAggregate
 * (TsdbQuery.java:294-363) and computeTags (SpanGroup.java:149-173) of every
 * group, from the spans' row keys.
 *
 * Input: the row keys of the spans in findSpans' TreeMap order, i.e. strictly
 * increasing under SpanCmp (TsdbQuery.java:594-621: metric bytes, then
 * everything after the 4 base-time bytes, unsigned, the shorter key first on
 * a common prefix). Two adjacent keys that are equal under SpanCmp (also: that
 * differ only in base time) or out of order: TSDBHIP_E_UNSORTED, the message
 * names the first offending span. A key shorter than metric_width + 4, whose
 * tag part is no multiple of name_width + value_width or holds more than
 * TSDBHIP_MAX_TAGS pairs, a key_off that decreases or does not end at
 * key_nbytes, group_bys not strictly ascending, a width outside 1..8 or
 * n_group_bys > TSDBHIP_MAX_TAGS: TSDBHIP_E_INVALID_ARG. Tag names inside a
 * key need not be sorted: the lookup is Tags.getValueId's linear scan, the
 * first match wins.
 *
 * Output: groups in ByteMap order (unsigned lexicographic) of their keys, a
 * group's key being the value ids of the group_bys tags in group_bys order;
 * the spans of a group in input order. A span lacking a group_bys tag is
 * dropped (TsdbQuery.java:339-344) and counted. n_group_bys == 0: one group of
 * every span, key of length 0 (TsdbQuery.java:298-309). n_spans == 0: no
 * group. A group exists even when span_kept clears all its spans (the
 * reference constructs the SpanGroup before SpanGroup.add filters); its
 * group_ntags is 0.
 *
 * Tags: group_tags holds the (name value) pairs of the group's first kept
 * span in key order; bit i of group_common is set iff every other kept span
 * of the group has pair i's name with pair i's value: SpanGroup.getTags() is
 * the pairs whose bit is set, getAggregatedTags() the names of the others (in
 * key order; the reference's HashSet has no defined order). A name only later
 * spans carry is reported nowhere, as in the reference. A key that repeats a
 * tag name: unspecified.
 *
 * n_groups > group_capacity: TSDBHIP_E_CAPACITY with n_groups, n_grouped and
 * n_dropped set and no array written. tsdbhip_last_timing: total_ms, hot_ms
 * (the sort passes), hot_kernel = TSDBHIP_HOT_GROUPBY, n_grid = the number of
 * sort passes run, alg_bytes = key bytes read + output bytes written. A
 * multi-device context runs the call on its first device.
 */
#define TSDBHIP_MAX_TAGS 8            /* Const.MAX_NUM_TAGS */

typedef struct tsdbhip_keys_desc {
  uint32_t flags;            /* TSDBHIP_DESC_DEVICE: key_off, key_bytes, span_kept are device pointers */
  uint32_t n_spans;
  uint8_t  metric_width, name_width, value_width;   /* each 1..8 (UniqueId widths) */
  uint8_t  n_group_bys;      /* 0..TSDBHIP_MAX_TAGS; 0 = no GROUP BY (TsdbQuery.java:298-309) */
  uint32_t reserved0;
  const uint64_t* key_off;   /* [n_spans+1]; span s's row key is key_bytes[key_off[s], key_off[s+1]) */
  const uint8_t*  key_bytes; /* full row keys: metric | base_time(4) | (name value)*; base time ignored */
  uint64_t        key_nbytes;
  const uint8_t*  span_kept; /* [n_spans] or NULL (all kept): SpanGroup.add's time filter, by the caller */
  const uint8_t*  group_bys; /* HOST always: n_group_bys * name_width bytes, strictly ascending (unsigned) */
} tsdbhip_keys_desc;

typedef struct tsdbhip_groups_out {   /* every array is a HOST array owned by the caller */
  uint32_t  group_capacity;  /* in */
  uint32_t  n_groups;        /* out; also set on TSDBHIP_E_CAPACITY so the caller can retry */
  uint32_t  n_grouped;       /* out: spans placed in some group */
  uint32_t  n_dropped;       /* out: spans lacking a group_by tag (TsdbQuery.java:339-344) */
  uint32_t* order;           /* [n_spans]: span indices in batch order, first n_grouped valid */
  uint32_t* group_span_start;/* [group_capacity+1]: exactly what tsdbhip_spangroup_run_batch takes */
  uint8_t*  group_key;       /* [group_capacity * n_group_bys*value_width] the ByteMap keys */
  uint8_t*  group_ntags;     /* [group_capacity] tag count of the group's first kept span; 0 if none kept */
  uint8_t*  group_tags;      /* [group_capacity * TSDBHIP_MAX_TAGS*(name_width+value_width)] that span's pairs */
  uint8_t*  group_common;    /* [group_capacity] bit i set: pair i is in every kept span of the group */
} tsdbhip_groups_out;

int tsdbhip_groupby_plan(tsdbhip_ctx* ctx, const tsdbhip_keys_desc* keys, tsdbhip_groups_out* out);

/*
 * The spans order[0..n) of the device-resident descriptor `in`
 * (TSDBHIP_DESC_DEVICE, else TSDBHIP_E_INVALID_ARG: a host descriptor is
 * repacked by its packer) as a descriptor of their own, in that order: the
 * batch order tsdbhip_groupby_plan returns. `out` receives the query fields
 * and flags of `in`, n_spans = n, n_rows = the gathered row count;
 * span_row_start and the five row_* arrays are new device arrays owned by
 * ctx (tsdbhip_desc_gather_free releases them and zeroes the pointers; a
 * second call is harmless). qual_bytes / val_bytes are BORROWED from `in`
 * (a row's offsets stay valid; they no longer grow with the row index): `in`
 * must outlive `out`. order is a host array; order[i] >= in->n_spans:
 * TSDBHIP_E_INVALID_ARG. Not with TSDBHIP_SHARDED.
 */
int tsdbhip_desc_gather(tsdbhip_ctx* ctx, const tsdbhip_sg_desc* in, const uint32_t* order,
                        uint32_t n, tsdbhip_sg_desc* out);
int tsdbhip_desc_gather_free(tsdbhip_ctx* ctx, tsdbhip_sg_desc* out);

/* ---- findSpans: the spans of a scan (an addition to ABI v8) -------------- */
/*
 * tsdbhip_find_spans: the TreeMap<byte[], Span> under SpanCmp that
 * TsdbQuery.findSpans fills row by row (TsdbQuery.java:240-285, 594-621), for
 * the rows a scanner delivered, in delivery order (HBase delivers in full-key
 * order; any order is accepted, as by the reference).
 *
 * Spans: one per distinct key under SpanCmp (metric bytes, then everything
 * after the 4 base-time bytes), in SpanCmp order: unsigned bytes, the shorter
 * key first on a common prefix. A span's key is the full row key of the first
 * delivered row of that span, with that row's base time (what TreeMap.put
 * keeps, :259-263; tsdbhip_groupby_plan ignores the base time). A row whose
 * row_status is TSDBHIP_ROW_NONE is one for which tsdb.compact(row) returned
 * null (:264-268): its span is still created, the row can be the one that
 * gives the span its key, and the row is not added to the span, so a span can
 * end up with no rows.
 *
 * Rows: the rows of a span keep delivery order (they are not sorted by time).
 * Whether a row is merged, dropped or rejected is Span.addRow's business
 * (Span.java:87-132): the SpanGroup entry points apply those rules to the
 * descriptor they get. The five row_* outputs and span_row_start are the six
 * arrays of a tsdbhip_sg_desc whose qual_bytes / val_bytes are the buffers the
 * scan's offsets point into (for a compacted scan: tsdbhip_rows_out's);
 * key_off / key_bytes are what tsdbhip_keys_desc takes.
 *
 * Errors: only the first offending row in delivery order counts, the message
 * names it, and no output array is written. A key not starting with `metric`:
 * TSDBHIP_E_ILLEGAL_DATA (:254-258). row_status TSDBHIP_ROW_ERROR:
 * TSDBHIP_E_ILLEGAL_DATA (the exception tsdb.compact throws inside findSpans);
 * TSDBHIP_ROW_OOB: TSDBHIP_E_OUT_OF_BOUNDS. On one row the metric check comes
 * first, as in the reference. Not reference behaviour, TSDBHIP_E_INVALID_ARG
 * (on one row before the two above): a width outside 1..8; a key shorter than
 * metric_width + 4, whose tag part is no multiple of name_width + value_width
 * or holds more than TSDBHIP_MAX_TAGS pairs; key_off decreasing or not ending
 * at key_nbytes (the latter before any row); a row_status above
 * TSDBHIP_ROW_OOB; for a row that is added, an odd row_qual_len or an odd
 * row_qual_off (the tsdbhip_sg_desc rule, checked here so that a bad offset
 * never reaches a decode kernel); a null required array; some but not all of
 * the scan's four cell arrays. A host descriptor is checked on the host before
 * anything is staged, a device descriptor by the first kernel, which proves
 * every key byte inside key_bytes before reading it.
 *
 * No row added at all (the reference returns null, :281-283), also
 * n_rows == 0: TSDBHIP_OK with n_spans = 0 and n_rows = 0; span_row_start[0]
 * and key_off[0] are set to 0 when the arrays are given.
 *
 * n_spans > span_capacity, or the span keys needing more than key_capacity:
 * TSDBHIP_E_CAPACITY with n_spans, n_rows, n_skipped and key_used set for a
 * retry and no array written.
 *
 * tsdbhip_last_timing: total_ms, hot_ms (the sort passes), hot_kernel =
 * TSDBHIP_HOT_FIND_SPANS, n_grid = the number of sort passes run (one per key
 * digit position that differs between rows), alg_bytes = bytes read plus bytes
 * written. A multi-device context runs the call on its first device.
 */
#define TSDBHIP_HAS_FIND_SPANS 1

typedef struct tsdbhip_scan_desc {
  uint32_t flags;             /* TSDBHIP_DESC_DEVICE: every array here AND in tsdbhip_spans_out is a
                                 device pointer; otherwise all are host pointers */
  uint32_t n_rows;
  uint8_t  metric_width, name_width, value_width, reserved0;
  uint32_t reserved1;
  const uint8_t*  metric;       /* HOST always: metric_width bytes, the query's metric */
  const uint64_t* key_off;      /* [n_rows+1] row r's key is key_bytes[key_off[r], key_off[r+1]) */
  const uint8_t*  key_bytes;    /* metric | base_time(4, big-endian) | (name value)* */
  uint64_t        key_nbytes;
  const uint8_t*  row_status;   /* [n_rows] TSDBHIP_ROW_* as tsdbhip_compact_rows wrote them, or NULL:
                                   every row is added */
  /* the compacted cell of each row, as tsdbhip_rows_out lays it out; all four NULL: only the
     order, the span boundaries and the keys are produced */
  const uint64_t* row_qual_off; /* [n_rows] */
  const uint32_t* row_qual_len; /* [n_rows] bytes */
  const uint64_t* row_val_off;  /* [n_rows] */
  const uint32_t* row_val_len;  /* [n_rows] */
} tsdbhip_scan_desc;

typedef struct tsdbhip_spans_out {
  uint32_t  span_capacity;     /* in */
  uint32_t  n_spans;           /* out (also on E_CAPACITY) */
  uint32_t  n_rows;            /* out: rows added (the reference's nrows) */
  uint32_t  n_skipped;         /* out: rows with status NONE */
  uint64_t  key_capacity;      /* in: bytes in key_bytes (key_nbytes of the input always suffices) */
  uint64_t  key_used;          /* out */
  uint32_t* row_order;         /* [scan n_rows] delivery index of output row i; first n_rows valid */
  uint64_t* span_row_start;    /* [span_capacity+1] */
  uint32_t* row_base;          /* [scan n_rows] base time read from the row key */
  uint32_t* row_ncells;        /* row_qual_len / 2 */
  uint64_t* row_qual_off;      /* passed through: the byte buffers are the caller's, untouched */
  uint64_t* row_val_off;
  uint32_t* row_val_len;
  uint64_t* key_off;           /* [span_capacity+1] } exactly what tsdbhip_keys_desc takes */
  uint8_t*  key_bytes;         /* [key_capacity]    } */
} tsdbhip_spans_out;

int tsdbhip_find_spans(tsdbhip_ctx* ctx, const tsdbhip_scan_desc* scan, tsdbhip_spans_out* out);

/* ---- getScanner: the rows of a query (an addition to ABI v8) ------------- */
/*
 * tsdbhip_scan_rows: the rows of a table that the Scanner of
 * TsdbQuery.getScanner (TsdbQuery.java:368-394) delivers: those inside its
 * start / stop keys (:378-388, getScanStartTime / getScanEndTime :396-425)
 * whose key matches the regexp of createAndSetFilter (:433-492), which holds
 * the fixed tags, the tag=* group-bys and the tag=v1|v2|... value lists of
 * findGroupBys (:192-223). The selection is what tsdbhip_find_spans takes.
 *
 * Table: a tsdbhip_scan_desc, host or device resident (TSDBHIP_DESC_DEVICE).
 * metric is the query's metric; rows may belong to any metric and come in any
 * order; row_status and the four cell arrays (all or none) are optional and
 * only gathered: row_status is passed through unread, the status and cell
 * checks stay tsdbhip_find_spans' business.
 *
 * Key range, in 64 bits and then truncated as the reference's (int) does:
 * scan_start = max(0, start_time - 2*3600 - sample_interval), scan_stop = the
 * low 32 bits of end_time + 3600 + 1 + sample_interval, or 0xFFFFFFFF with
 * TSDBHIP_SCAN_END_UNSET. A row is in range iff start_key <= key < stop_key,
 * the keys being metric | time (big-endian), compared as HBase does: unsigned
 * bytes, the shorter key first. For a well-shaped key: its metric bytes are
 * the query's and scan_start <= base_time < scan_stop, unsigned. The wrap is
 * reference behaviour: an end_time near 2^32 gives a stop below the start and
 * selects nothing. A row of another metric is not selected; it is no error.
 *
 * Tag filter, applied only if n_tags + n_group_bys > 0: the items are the tags
 * and group-bys merged in ascending name order (:455-488). The key's tag part
 * must contain pairs, in that order, where pair i has item i's name and item
 * i's value: the value of a fixed tag, any value for a group-by without value
 * ids, one of the listed ids otherwise; any number of other pairs may stand
 * before, between and after them ("(?:.{pair})*"). That is the regexp's
 * language: a key's at most TSDBHIP_MAX_TAGS pairs are walked once, an item
 * cursor advancing on the earliest match. The Java `$` may also match before
 * a final line terminator (under ISO-8859-1 also 0x0D, 0x85 and \r\n); the
 * rest of the pattern then has to cover a tag part that is one or two bytes
 * short of a multiple of the pair width, which it cannot, so for a key whose
 * tag part is a multiple of the pair width (the only keys accepted here) the
 * result is the same. More than TSDBHIP_MAX_TAGS items in all: a valid query
 * that matches no row.
 *
 * Errors, TSDBHIP_E_INVALID_ARG: a width outside 1..8; some but not all of
 * the four cell arrays; a null required array; n_tags or n_group_bys above
 * TSDBHIP_MAX_TAGS; tags or group_bys not strictly ascending by name; a name
 * in both (the reference's AssertionError, :510-515); a null tags / group_bys
 * / value array that the counts need. Then the key rules of
 * tsdbhip_find_spans, over every row of the table, selected or not: key_off
 * not ending at key_nbytes (before any row), decreasing or past key_nbytes; a
 * key shorter than metric_width + 4, whose tag part is no multiple of
 * name_width + value_width or holds more than TSDBHIP_MAX_TAGS pairs. Only
 * the first offending row in table order counts, the message names it, and
 * nothing is written. A host table is checked on the host before anything is
 * staged, a device table by the match kernel, which proves every key byte
 * inside key_bytes before reading it.
 *
 * Output: the selected rows in table order; the arrays are what a second
 * tsdbhip_scan_desc takes (n_rows = n_selected, key_nbytes = key_used), so
 * tsdbhip_find_spans runs on them unchanged. Cell offsets are passed through:
 * cell bytes are never copied. row_capacity < n_selected or key_capacity <
 * key_used: TSDBHIP_E_CAPACITY with both counts set for a retry and no array
 * written. Nothing selected, also n_rows == 0: TSDBHIP_OK, the counts 0 and
 * key_off[0] = 0 (when the array is given). For a device table every output
 * is a device pointer, written in place; for a host table the outputs are
 * host arrays.
 *
 * Value lists of any length (1024 ids and more) are fine; duplicates are
 * allowed. tsdbhip_set_option: "scan_rows_load" "auto" | "lanes" | "lds" how
 * the match kernel reads the keys (a lane its own key byte by byte, or a wave
 * the contiguous keys of its 64 rows in 16-byte pieces through LDS; "auto":
 * "lds"), "scan_rows_blocks" "auto" | a positive count: that kernel's
 * grid at most (its waves stride over the table). Results never depend on
 * either.
 *
 * tsdbhip_last_timing: total_ms, hot_ms (the match kernel), hot_kernel =
 * TSDBHIP_HOT_SCAN_ROWS, alg_bytes = bytes read plus bytes written. A
 * multi-device context runs the call on its first device.
 */
#define TSDBHIP_HAS_SCAN_ROWS 1
#define TSDBHIP_HOT_SCAN_ROWS 12     /* k_sr_match: range and tag filter over every key of the table */
#define TSDBHIP_SCAN_END_UNSET 0x1u  /* tsdbhip_scan_query.flags: end_time == UNSET, scan to 0xFFFFFFFF */

typedef struct tsdbhip_scan_query {  /* every pointer is HOST memory */
  uint32_t start_time, end_time;     /* getStartTime() / getEndTime(), seconds */
  uint32_t sample_interval;          /* 0: none */
  uint32_t flags;                    /* TSDBHIP_SCAN_END_UNSET */
  uint32_t n_tags;                   /* 0..TSDBHIP_MAX_TAGS */
  uint32_t n_group_bys;              /* 0..TSDBHIP_MAX_TAGS */
  const uint8_t*  tags;              /* n_tags * (name_width + value_width): (name value), strictly ascending by name */
  const uint8_t*  group_bys;         /* n_group_bys * name_width: names, strictly ascending */
  const uint32_t* group_by_nvalues;  /* [n_group_bys] value ids of that group-by; 0: any value. NULL: all 0 */
  const uint8_t*  group_by_values;   /* the ids, value_width bytes each, concatenated in group_bys order */
} tsdbhip_scan_query;

typedef struct tsdbhip_scan_sel {
  uint32_t  row_capacity;      /* in */
  uint32_t  n_selected;        /* out (also on E_CAPACITY) */
  uint64_t  key_capacity;      /* in: bytes in key_bytes (key_nbytes of the table always suffices) */
  uint64_t  key_used;          /* out (also on E_CAPACITY) */
  uint32_t* row_index;         /* [row_capacity] index into the table of selected row i */
  uint64_t* key_off;           /* [row_capacity+1] } what tsdbhip_scan_desc takes */
  uint8_t*  key_bytes;         /* [key_capacity]   } */
  uint8_t*  row_status;        /* [row_capacity] gathered if the table has it, else ignored */
  uint64_t* row_qual_off;      /* [row_capacity] the four cell arrays likewise */
  uint32_t* row_qual_len;
  uint64_t* row_val_off;
  uint32_t* row_val_len;
} tsdbhip_scan_sel;

int tsdbhip_scan_rows(tsdbhip_ctx* ctx, const tsdbhip_scan_desc* table, const tsdbhip_scan_query* query,
                      tsdbhip_scan_sel* out);

/* ---- repacking device rows to the streaming layout (an addition to ABI v8) - */
/*
 * tsdbhip_desc_pack: the spans order[0..n) of the device-resident descriptor
 * `in`, like tsdbhip_desc_gather, with their rows' bytes COPIED into new
 * buffers in packing.pack_spans' layout: the layout the streaming kernels take
 * (qualifiers at 0 mod 8, values at 0 mod 16; see tsdbhip_sg_desc), which
 * tsdbhip_compact_rows' placement and a gathered descriptor miss.
 *
 * Input: `in` must be device resident (TSDBHIP_DESC_DEVICE) and not
 * TSDBHIP_SHARDED, and in != out; else TSDBHIP_E_INVALID_ARG. order is a host
 * array of n span indices, order[i] >= in->n_spans: TSDBHIP_E_INVALID_ARG; a
 * span may appear more than once. order == NULL: every span of `in` in its own
 * order, and n must equal in->n_spans.
 *
 * Output: `out` receives the query fields and flags of `in`, n_spans = n,
 * n_rows = the gathered row count, span0 = 0. span_row_start, row_base,
 * row_ncells and row_val_len are what tsdbhip_desc_gather returns for the same
 * arguments. Gathered row i lies at
 *   row_qual_off[i] = sum over j < i of align8(2 * row_ncells[j])
 *   row_val_off[i]  = sum over j < i of align16(row_val_len[j])     (64 bits)
 * and qual_nbytes = align16(max(sum of align8, 1)), val_nbytes likewise from
 * the sum of align16. Every row's bytes are copied unchanged, every byte of
 * [0, nbytes) outside a row is 0, and the allocations are readable and zero
 * for 64 bytes past nbytes: the eight arrays are byte for byte what
 * packing.pack_spans returns for the same rows. All eight are new device
 * allocations owned by ctx; `out` needs nothing from `in` afterwards.
 * tsdbhip_desc_pack_free releases them and zeroes the eight pointers and the
 * two nbytes; a second call is harmless. (tsdbhip_desc_gather_free does not
 * release a packed descriptor.) Packing into an `out` that already holds a
 * packed descriptor releases the earlier one once the new one stands.
 *
 * Source rows may lie at any offset, odd qualifier offsets included: this is a
 * byte copy. A gathered row with row_qual_off + 2 * row_ncells > in->qual_nbytes
 * or row_val_off + row_val_len > in->val_nbytes: TSDBHIP_E_INVALID_ARG; only the
 * first offending gathered row counts, the message names it, *out is left
 * untouched, and the check runs before any byte is read. The call reads
 * nothing before in->qual_bytes / in->val_bytes and nothing at or beyond
 * nbytes + 64 (the slack TSDBHIP_DESC_DEVICE requires), and never writes to
 * `in`.
 *
 * tsdbhip_set_option "desc_pack_load" "auto" | "unaligned" | "shift": how the
 * copy kernel loads a row's bytes: "unaligned", one 16-byte (qualifiers:
 * 8-byte) load at the row's own residue; "shift", dword-aligned loads and
 * v_alignbyte_b32 by the residue; "auto": "unaligned" (DESIGN.md). Results
 * never depend on it.
 *
 * tsdbhip_last_timing: total_ms, hot_ms (the copy kernel), hot_kernel =
 * TSDBHIP_HOT_DESC_PACK, alg_bytes = row bytes read + buffer bytes written +
 * metadata read and written. A multi-device context runs the call on its
 * first device.
 */
#define TSDBHIP_HAS_DESC_PACK 1
#define TSDBHIP_HOT_DESC_PACK 13   /* k_pack_copy */
int tsdbhip_desc_pack(tsdbhip_ctx* ctx, const tsdbhip_sg_desc* in, const uint32_t* order, uint32_t n,
                      tsdbhip_sg_desc* out);
int tsdbhip_desc_pack_free(tsdbhip_ctx* ctx, tsdbhip_sg_desc* out);

/* ---- the qualifier certificate of a resident descriptor (an addition to ABI v8) - */
/*
 * TSDBHIP_DESC_QUALS_PROVEN states, of a device descriptor: for every row with
 * row_ncells >= 2, qualifier c of the row, read as a big-endian 16-bit word,
 * equals q0 + c * (q1 - q0) without wrap (q0, q1: the row's first two
 * qualifiers), and q1 - q0 is positive and a multiple of 16. That is one flags
 * nibble for the whole row and a constant positive step in seconds, every
 * delta at most 4095. A row of one cell is trivially proven. The statement is
 * about the qualifier bytes alone, not about the cell type or the query.
 *
 * It is what the streaming kernels otherwise prove on every call by reading
 * every qualifier (a fifth of an 8-byte row's bytes). A compacted row of a
 * closed hour does not change between queries, so a resident table is proven
 * once: the direct aligned group (TSDBHIP_PATH_GROUP_DIRECT) then reads only
 * each row's fields, its first qualifier word and its values, and reports
 * TSDBHIP_PATH_QUALS_PROVEN. What depends on the query or on the other spans
 * (the class key, the cell width, the window, the bucket count) is still
 * checked on every call, and a group that fails there falls back as before;
 * the rerun from assembly proves what it reads.
 *
 * The flag is the caller's promise that the rows' qualifier bytes have not
 * changed since they were proven, as TSDBHIP_DESC_DEVICE is a promise about
 * the pointers: clear it, or certify again, when a row's bytes are rewritten
 * or the row arrays are changed. With a false promise the results are
 * undefined, but every access stays inside what the descriptor describes (the
 * addresses never depend on the qualifiers not read). The flag is ignored on a
 * host descriptor (flags without TSDBHIP_DESC_DEVICE) and by every path other
 * than the direct aligned group; "quals_proven" "off" ignores it everywhere.
 *
 * tsdbhip_desc_certify reads every row's qualifiers once (one kernel, a wave a
 * row at a time), counts the rows that fail the statement into
 * *n_unproven_rows (may be NULL), and sets the flag in desc->flags iff the
 * count is 0, else clears it. desc must be device resident, else
 * TSDBHIP_E_INVALID_ARG. A row with an odd row_qual_off or with row_qual_off +
 * 2 * row_ncells > qual_nbytes counts as unproven and none of its bytes is
 * read: no error is raised, the query itself reports errors. Any even
 * qualifier offset is taken. tsdbhip_last_timing: total_ms, hot_ms (the
 * kernel), hot_kernel = TSDBHIP_HOT_DESC_CERTIFY, alg_bytes = qual_nbytes + 12
 * B of metadata a row. A multi-device context runs the call on its first
 * device.
 *
 * Producers whose buffers the context owns run the same proof on what they
 * produced: tsdbhip_synth_generate after generation, tsdbhip_desc_pack after
 * its copy (an input that carries the flag hands it on without a second proof:
 * the copied bytes are the same bytes). tsdbhip_desc_gather's output carries
 * its input's flags: a selection of proven rows is proven.
 */
#define TSDBHIP_HAS_DESC_CERTIFY 1
#define TSDBHIP_HOT_DESC_CERTIFY 14   /* k_desc_certify */
int tsdbhip_desc_certify(tsdbhip_ctx* ctx, tsdbhip_sg_desc* desc, uint64_t* n_unproven_rows);

/* ---- output formatting (host cores, no GPU) ----------------------------- */
/*
 * Writes the text the reference's consumers print for n points of one
 * SpanGroup (tsdbhip_sg_out arrays) into buf:
 *   TSDBHIP_FMT_ASCII   "<metric> <ts> <value><tags>\n"   GraphHandler.respondAsciiQuery
 *                        (GraphHandler.java:785-808); tags = " k=v k2=v2" as the
 *                        caller built it from getTags()
 *   TSDBHIP_FMT_GNUPLOT "<ts + utc_offset> <value>\n"     Plot.dumpToFiles (Plot.java:190-204)
 *   TSDBHIP_FMT_CLI     "<metric> <ts> <value> <tags>\n"  CliQuery (CliQuery.java:161-170);
 *                        tags = getTags().toString(), doubles as String.format("%f")
 * Longs as Long.toString, doubles as Double.toString (JDK 19+ shortest
 * digits). Returns the bytes written, TSDBHIP_E_CAPACITY if cap is too small
 * (nothing written), TSDBHIP_E_NAN_INF for a NaN/Infinity in ASCII/GNUPLOT
 * (the reference's IllegalStateException), TSDBHIP_E_INVALID_ARG.
 */
#define TSDBHIP_FMT_ASCII   0
#define TSDBHIP_FMT_GNUPLOT 1
#define TSDBHIP_FMT_CLI     2
int64_t tsdbhip_format_points(int32_t mode, const char* metric, const char* tags, int64_t utc_offset,
                              const int64_t* ts, const uint8_t* is_int, const int64_t* bits, uint64_t n,
                              char* buf, uint64_t cap);

/* ---- secondary path ---------------------------------------------------- */
int tsdbhip_compact_rows(tsdbhip_ctx* ctx, const tsdbhip_rows_desc* desc,
                         tsdbhip_rows_out* out);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI -------------------- */
#define TSDBHIP_UNIQUE_ID_BYTES 128
int tsdbhip_comm_unique_id(uint8_t out[TSDBHIP_UNIQUE_ID_BYTES]);
int tsdbhip_comm_init(tsdbhip_ctx* ctx, int32_t nranks, int32_t rank,
                      const uint8_t id[TSDBHIP_UNIQUE_ID_BYTES]);

/* ---- device-resident synthetic SpanGroup ------------------------------- */
/* Generates the KeyValue bytes of a synthetic SpanGroup directly in HBM
 * (same bytes as opentsdb_amd.synth on the host) and fills *desc with device
 * pointers owned by ctx (flags |= TSDBHIP_DESC_DEVICE). Free with
 * tsdbhip_synth_free. Only n_spans/n_points/... of params are used; the
 * query fields of *desc (start/end/agg/...) are left for the caller. */
int tsdbhip_synth_generate(tsdbhip_ctx* ctx, const tsdbhip_synth_params* p,
                           tsdbhip_sg_desc* desc);
int tsdbhip_synth_free(tsdbhip_ctx* ctx, tsdbhip_sg_desc* desc);

/* Copies the device-resident desc's arrays back to host buffers sized by the
 * desc (for parity checks of the generator). */
int tsdbhip_desc_download(tsdbhip_ctx* ctx, const tsdbhip_sg_desc* ddesc,
                          uint64_t* span_row_start, uint32_t* row_base,
                          uint32_t* row_ncells, uint64_t* row_qual_off,
                          uint64_t* row_val_off, uint32_t* row_val_len,
                          uint8_t* qual_bytes, uint8_t* val_bytes);

/* ---- measurement ------------------------------------------------------- */
/* Bandwidth probe over a device-resident desc (TSDBHIP_DESC_DEVICE):
 * mode 0 streams its qualifier + value rows with the geometry of the
 * downsampling kernel (one wave per span, 16-B loads), mode 1 copies its
 * value bytes device-to-device, mode 2 is a flat grid-stride read of the
 * value bytes, mode 3 is mode 0 with two chunks in flight per wave and the
 * next span's metadata loaded ahead (width 8, single-row spans).
 * On mode 3's geometry: mode 4 reads the values in whole lines (instruction i
 * of a 512-cell chunk: lane l the 16 B at chunk + 1024 i + 16 l, 1 KB
 * contiguous a wave instruction, where mode 3's lanes read 64 B apart),
 * mode 5 is mode 3 with non-temporal loads, mode 6 mode 4 with them; mode 7
 * is mode 2 with non-temporal loads. Any other mode: TSDBHIP_E_INVALID_ARG.
 * *ms = kernel time, *bytes = bytes moved.
 * `width` = value bytes per cell (4 or 8). Not part of the reference API:
 * it reports the achievable bandwidth beside the 8 TB/s peak. */
int tsdbhip_bw_probe(tsdbhip_ctx* ctx, const tsdbhip_sg_desc* desc, int32_t mode, uint32_t width,
                     float* ms, uint64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* TSDBHIP_H */
