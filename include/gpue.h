/* gpue.h — C-ABI boundary of the MI355X-native execution engine for the
 * StarRocks BE hot path.
 *
 * These entry points are what thin C++ Operator wrappers inside the reference
 * BE would call from the pipeline driver loop
 * (reference be/src/exec/runtime/pipeline_driver.cpp:391-500); the mapping of
 * each entry to the reference interface it replaces is given per declaration.
 * INTEGRATION.md shows the Operator-side binding a maintainer would add.
 *
 * Conventions: extern "C"; plain pointers + sizes; opaque handles; int status
 * returns (0 == GPUE_OK, matching Status::ok() of reference
 * be/src/base/status.h); no torch types. The implementation (HIP/C++,
 * starrocks_amd/csrc/gpue.hip) FAILS at session creation when no AMD GPU is
 * present — there is no CPU fallback in the product path.
 */
#ifndef GPUE_H
#define GPUE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPUE_OK 0
#define GPUE_ERR_HIP 1        /* HIP runtime failure (details: gpue_last_error) */
#define GPUE_ERR_ARG 2        /* bad argument */
#define GPUE_ERR_NO_GPU 3     /* no AMD GPU visible */

/* Human-readable detail of the last non-OK status on this thread. */
const char* gpue_last_error(void);

/* ---- session ----
 * Engine lifetime per device; analog of FragmentExecutor::prepare/close
 * (reference be/src/orchestration/fragment_executor.h:40-42). One session ==
 * one HIP device + one HIP stream (one pipeline driver <-> one stream,
 * SURVEY.md §2 pipeline row). */
typedef struct gpue_session gpue_session;
int gpue_session_create(int device_index, gpue_session** out);
void gpue_session_destroy(gpue_session* s);
int gpue_device_count(int* out);
int gpue_sync(gpue_session* s);

/* ---- device buffers ----
 * Raw HBM allocations; the engine-side analog of Chunk column containers
 * (reference be/src/column/fixed_length_column_base.h:283) held resident on
 * device. Chunked Operator pushes append into these (gpue_dbuf_h2d with
 * dst_off). */
typedef struct gpue_dbuf gpue_dbuf;
int gpue_dbuf_alloc(gpue_session* s, uint64_t bytes, gpue_dbuf** out);
void gpue_dbuf_free(gpue_dbuf* b);
int gpue_dbuf_h2d(gpue_dbuf* b, const void* src, uint64_t bytes, uint64_t dst_off);
int gpue_dbuf_d2h(gpue_dbuf* b, void* dst, uint64_t bytes, uint64_t src_off);
int gpue_dbuf_memset(gpue_dbuf* b, int value, uint64_t bytes);
int gpue_dbuf_d2d(gpue_dbuf* src, gpue_dbuf* dst, uint64_t bytes, uint64_t src_off,
                  uint64_t dst_off);
/* SUM(a[i]*b[i]) + row count accumulated into acc (i64[2]) — the agg sink
 * update for the chunked (unfused) config-2 plan (Aggregator::update_batch
 * with sum<int64> states, reference be/src/exprs/agg/sum.h:45-181). */
int gpue_sum_prod_u32(gpue_session* s, gpue_dbuf* a, gpue_dbuf* b, uint64_t n,
                      gpue_dbuf* acc);

/* ---- hipGraph step replay ----
 * Capture the async launch sequence of one step between begin/end, then
 * replay it with a single hipGraphLaunch per step. Removes the per-launch
 * host cost that dominates small (SF10-sized) steps; the CDNA-native analog
 * of the reference driver's time-slice batching. Only stream-async entries
 * (the *_async pipelines, memsets) may sit inside a capture. */
typedef struct gpue_graph gpue_graph;
int gpue_graph_begin(gpue_session* s);
int gpue_graph_end(gpue_session* s, gpue_graph** out);
int gpue_graph_launch(gpue_session* s, gpue_graph* g);
void gpue_graph_destroy(gpue_graph* g);
/* Wrap external device memory (e.g. a torch tensor's data_ptr) so kernels
 * operate in place and torch.distributed (RCCL) moves the same buffers —
 * the all-to-all leg of configs 4-5. Caller keeps ownership. */
int gpue_dbuf_wrap(gpue_session* s, void* device_ptr, uint64_t bytes, gpue_dbuf** out);
/* Expose the device pointer (torch interop / sub-buffer views). */
int gpue_dbuf_ptr(gpue_dbuf* b, void** out);

/* ---- synthetic chunk source ----
 * Replaces the scan operator with a seeded on-device generator (SURVEY.md §2
 * scan row: storage engine OUT OF SCOPE, synthetic source instead). The
 * generator (splitmix64 finalizer on row index) is bit-identical to
 * oracle/oracle.c orc_gen_* and tests' numpy restatement. */
int gpue_gen_u32_mod(gpue_session* s, gpue_dbuf* out, uint64_t seed, uint64_t tag,
                     uint64_t row_start, uint64_t n, uint32_t mod, uint32_t add);
int gpue_gen_i64(gpue_session* s, gpue_dbuf* out, uint64_t seed, uint64_t tag,
                 uint64_t row_start, uint64_t n);
/* SSB lineorder column sets (schema: reference test/common/sql/ssb/create.sql) */
int gpue_gen_lineorder_q1(gpue_session* s, uint64_t seed, uint64_t row_start, uint64_t n,
                          gpue_dbuf* lo_orderdate, gpue_dbuf* lo_extendedprice,
                          gpue_dbuf* lo_discount);
int gpue_gen_lineorder_q21(gpue_session* s, uint64_t seed, uint64_t row_start, uint64_t n,
                           gpue_dbuf* lo_partkey, gpue_dbuf* lo_suppkey,
                           gpue_dbuf* lo_orderdate, gpue_dbuf* lo_revenue);
int gpue_gen_lineorder_q43(gpue_session* s, uint64_t seed, uint64_t row_start, uint64_t n,
                           gpue_dbuf* lo_custkey, gpue_dbuf* lo_suppkey,
                           gpue_dbuf* lo_partkey, gpue_dbuf* lo_orderdate,
                           gpue_dbuf* lo_revenue, gpue_dbuf* lo_supplycost);

/* ---- scan + predicate filter ----
 * Replaces ChunkPredicateEvaluator::eval_conjuncts + Column::filter_range
 * (reference be/src/exprs/chunk_predicate_evaluator.cpp:31-80,
 * be/src/base/simd/filter.h:26-38). Ordered (stable) compaction of int64
 * values v < theta; output order bit-identical to the reference loop. */
int gpue_scan_filter_i64_lt(gpue_session* s, gpue_dbuf* in, uint64_t n, int64_t theta,
                            gpue_dbuf* out, uint64_t* out_count);
/* Single-pass variant (decoupled lookback): one coalesced read + one
 * coalesced write per element — the reference's algorithmic byte count. */
int gpue_scan_filter_i64_lt_sp(gpue_session* s, gpue_dbuf* in, uint64_t n, int64_t theta,
                               gpue_dbuf* out, uint64_t* out_count);

/* Multi-conjunct predicate evaluation with the reference's eager-prune
 * strategy (chunk_predicate_evaluator.cpp:31-80: AND-merge per conjunct,
 * all-true skip, all-false short-circuit, compact all columns when zeros
 * exceed max(0.8*rows, 1024)). preds are (col_index, op, lo, hi) arrays;
 * op: 0 EQ(lo), 1 LT(hi), 2 BETWEEN[lo,hi]. Columns compact stably in
 * place; out_rows = survivors. */
int gpue_eval_conjuncts_i32(gpue_session* s, gpue_dbuf** cols, int n_cols, uint64_t n_rows,
                            const int32_t* pred_col, const int32_t* pred_op,
                            const int32_t* pred_lo, const int32_t* pred_hi, int n_preds,
                            uint64_t* out_rows);
int gpue_eval_conjuncts_i64(gpue_session* s, gpue_dbuf** cols, int n_cols, uint64_t n_rows,
                            const int32_t* pred_col, const int32_t* pred_op,
                            const int64_t* pred_lo, const int64_t* pred_hi, int n_preds,
                            uint64_t* out_rows);

/* ---- predicate expressions ----
 * Replaces ChunkPredicateEvaluator::eval_conjuncts over compound, IN and null
 * predicates (reference be/src/exprs/chunk_predicate_evaluator.cpp:31-80 with
 * compound_predicate / in_const_predicate / is_null_predicate children) plus
 * Column::filter_range: a whole OR/NOT/IN/IS NULL tree over int32 and int64
 * columns, nullable or not, is evaluated in ONE pass into a selection bitmap
 * (gpue_pred_eval_mask); gpue_mask_compact then compacts any columns by a
 * bitmap. The reference's per-conjunct u8 Filter vector shrinks to one bit
 * per row; gpue_eval_conjuncts_* and gpue_scan_filter_* are unchanged.
 *
 * The program is postfix (reverse Polish) over parallel arrays (op, col, a,
 * b), the convention gpue_eval_conjuncts_* uses for its predicates. A leaf
 * pushes one value, a connective pops its operands and pushes the result; the
 * root is the one value left.
 *
 * Semantics are SQL three-valued logic — what the reference's evaluator
 * yields once a nullable result column is folded into the filter (filter =
 * data & !null). An I32 column value is sign-extended to int64 and compared
 * against a / b as int64 (so col < 2^40 on an I32 column is TRUE for every
 * non-NULL row); all compares are signed. A compare, BETWEEN or IN leaf on a
 * NULL row is UNKNOWN; with GPUE_P_RHS_COL it is UNKNOWN if either side is
 * NULL, and the two columns must have the same pred_type. IS_NULL is TRUE or
 * FALSE, never UNKNOWN, and FALSE on a column without a null mask. The value
 * stored under a NULL row is never read into the result. AND / OR / NOT are
 * Kleene: AND is F if either operand is F, T if both are T, else U; OR is T
 * if either is T, F if both are F, else U; NOT swaps T and F and keeps U. IN
 * with b == 0 is FALSE on non-NULL rows, UNKNOWN on NULL rows; IN lists may be
 * unsorted and hold duplicates (the host sorts and de-duplicates before
 * upload). A row's bit is set iff the root is TRUE. mask holds ceil(n_rows/64)
 * u64 words, bit (r & 63) of word r >> 6 = row r; bits of the last word at
 * positions >= n_rows are written as 0. out_count = set bits.
 *
 * Strings are deliberately not a leaf type: a varchar predicate is lowered by
 * the caller to EQ / IN / BETWEEN over dictionary codes (the engine already
 * decodes dict pages to int32 codes, gpue_page_decode_*).
 *
 * GPUE_ERR_ARG, before any launch or allocation, for: n_insns outside
 * 1..GPUE_PRED_MAX_INSNS; an unknown op; stack underflow; stack depth above
 * GPUE_PRED_MAX_STACK; final stack depth other than 1; a column index out of
 * range (the RHS_COL index in `a` included); an RHS_COL type mismatch; RHS_COL
 * on a non-compare op; an IN range outside [0, n_in_values]; an unknown
 * pred_type; n_rows >= 2^32; a column or null buffer shorter than n_rows
 * elements; a mask shorter than ceil(n_rows/64)*8 bytes. n_rows == 0 returns
 * GPUE_OK with count 0. */
/* pred column types */
#define GPUE_PT_I32 0
#define GPUE_PT_I64 1
/* leaf ops: push one value. `col` = predicate-column index. */
#define GPUE_P_EQ 0   /* col == a */
#define GPUE_P_NE 1
#define GPUE_P_LT 2
#define GPUE_P_LE 3
#define GPUE_P_GT 4
#define GPUE_P_GE 5
#define GPUE_P_BETWEEN 6   /* a <= col <= b */
#define GPUE_P_IN 7        /* col in in_values[a .. a+b) */
#define GPUE_P_IS_NULL 8
/* connectives: pop operands, push result */
#define GPUE_P_AND 16
#define GPUE_P_OR 17
#define GPUE_P_NOT 18
/* OR-ed into a compare op (EQ..GE): `a` is a second predicate-column index */
#define GPUE_P_RHS_COL 0x100
#define GPUE_PRED_MAX_INSNS 64
#define GPUE_PRED_MAX_STACK 16
int gpue_pred_eval_mask(gpue_session* s,
                        gpue_dbuf** pred_cols,
                        gpue_dbuf** pred_nulls, /* entries may be NULL; u8, nonzero = NULL row */
                        const int32_t* pred_type, int n_pred_cols,
                        const int32_t* insn_op, const int32_t* insn_col,
                        const int64_t* insn_a, const int64_t* insn_b, int n_insns,
                        const int64_t* in_values, /* host; may be NULL when n_in_values == 0 */
                        uint64_t n_in_values,
                        uint64_t n_rows,
                        gpue_dbuf* mask,        /* ceil(n_rows/64) u64 words */
                        uint64_t* out_count);
/* Stable compaction of any columns by a bitmap in gpue_pred_eval_mask's
 * format: survivors keep ascending row order, so the output is bit-identical
 * to the reference's filter_range loop (be/src/base/simd/filter.h:26-38).
 * Bits of the last word at positions >= n_rows are ignored even if the caller
 * left garbage there. col_width is 1, 4 or 8 bytes per column — width 1 so a
 * nullable column's u8 null mask travels with it. out_row_idx (nullable)
 * receives the surviving row indices as ascending u32. With n_cols == 0 and
 * out_row_idx == NULL the call is a count-only popcount of the mask.
 * Two phases, no workgroup waits on another: per-tile popcounts, a block scan
 * of the tile counts, then the emit. After the scan the count is known and
 * *out_count is set; a dst_cols[k] shorter than count*width bytes or an
 * out_row_idx shorter than count*4 bytes then returns GPUE_ERR_ARG with
 * *out_count valid, so the caller can size and retry. GPUE_ERR_ARG also for
 * src == dst for any column, any dst (or out_row_idx) overlapping a src, the
 * mask or another dst of the same call, a width outside {1, 4, 8}, a src
 * shorter than n_rows*width bytes, a mask shorter than ceil(n_rows/64)*8
 * bytes, and n_rows >= 2^32. */
int gpue_mask_compact(gpue_session* s, gpue_dbuf* mask, uint64_t n_rows,
                      gpue_dbuf** src_cols, gpue_dbuf** dst_cols,
                      const int32_t* col_width /* 1, 4 or 8 bytes */, int n_cols,
                      gpue_dbuf* out_row_idx /* nullable; u32 surviving row indices, ascending */,
                      uint64_t* out_count);

/* ---- scalar expressions ----
 * The Project step: ExprContext::evaluate over arithmetic, cast and
 * conditional expressions (reference be/src/exprs/arithmetic_expr.cpp,
 * cast_expr.cpp, condition_expr.cpp), run between scan/filter and join/agg.
 * ONE pass over the input columns evaluates up to GPUE_EXPR_MAX_OUT
 * expressions and writes every output column. Same machine as the predicate
 * section with a value stack in place of the truth stack; no existing entry
 * changes.
 *
 * The program is postfix over parallel arrays (op, col, a): at most
 * GPUE_EXPR_MAX_INSNS instructions, stack depth at most GPUE_EXPR_MAX_STACK.
 * Every stack value is an int64 plus a NULL flag. I32 columns are
 * sign-extended on load; a row is NULL iff its in_nulls byte is nonzero, and
 * the value stored under an input NULL row is never read into a result.
 *
 * Leaves: X_COL pushes input column `col`, X_CONST pushes `a`, X_NULL the
 * NULL literal. Unary: X_NEG, X_ABS (two's-complement wrapping:
 * ABS(INT64_MIN) = INT64_MIN), X_NOT (1 if the value is 0, else 0),
 * X_IS_NULL (1 or 0, never NULL), X_CAST_I32 (a value outside the int32 range
 * becomes NULL, the reference's cast-overflow result). Binary, left operand
 * pushed first: X_ADD / X_SUB / X_MUL wrap; X_DIV truncates toward zero, a
 * zero divisor gives NULL, INT64_MIN / -1 gives INT64_MIN; X_MOD takes the
 * sign of the dividend, a zero divisor gives NULL, x % -1 gives 0.
 * GPUE_X_CHECKED OR-ed into ADD, SUB, MUL, NEG or ABS turns signed overflow
 * into NULL — the decimal64 overflow-to-NULL mode (decimals are scaled int64;
 * the caller owns the scale). NULL in gives NULL out for all of these.
 * X_EQ..X_GE compare two stack values, signed: 1 or 0, NULL if either side
 * is NULL. X_AND / X_OR are Kleene as in the predicate section, over nonzero
 * = TRUE, zero = FALSE; the result is 1, 0 or NULL. X_IF pops else, then,
 * cond and yields `then` iff cond is non-NULL and nonzero, otherwise `else`
 * (CASE WHEN chains lower to nested IF; a missing ELSE is X_NULL). X_IFNULL
 * pops b, a and yields a unless it is NULL, otherwise b. X_OUT pops the top
 * of the stack into output `col`; the stack must be empty after each X_OUT,
 * every output index in [0, n_out) is written exactly once, and the program
 * ends with an X_OUT.
 *
 * Outputs: XO_I64 stores the value, XO_I32 its low 32 bits (a checked
 * narrowing is X_CAST_I32), XO_MASK a bitmap in exactly gpue_pred_eval_mask's
 * format — a row's bit is set iff the value is non-NULL and nonzero, trailing
 * bits of the last word are 0 — which feeds gpue_mask_compact directly. The
 * value stored under a NULL row is 0 and out_nulls[k][row] is 1 or 0, so
 * whole buffers compare bit-exactly. out_nulls[k] of an XO_MASK output is
 * ignored.
 *
 * Static nullability, computed on the host while validating: X_COL is
 * nullable iff the column has a null mask; X_NULL, DIV, MOD, CAST_I32 and
 * checked ops are nullable; IS_NULL is not; IFNULL is nullable iff b is; IF
 * iff then or else is; every other op iff any operand is.
 *
 * GPUE_ERR_ARG, before any launch or allocation, for: n_insns outside
 * 1..GPUE_EXPR_MAX_INSNS, n_out outside 1..GPUE_EXPR_MAX_OUT, n_in_cols
 * outside 0..GPUE_EXPR_MAX_IN_COLS; an unknown op or flag, or CHECKED on an
 * op that does not take it; stack underflow, depth above GPUE_EXPR_MAX_STACK,
 * or a non-empty stack after an OUT; a program that does not end with an OUT;
 * an output written twice or never; a column or output index out of range; an
 * unknown in_type / out_type; a nullable expression whose out_nulls[k] is
 * NULL (XO_MASK outputs excepted); n_rows >= 2^32; any buffer shorter than
 * n_rows elements (a mask: ceil(n_rows/64)*8 bytes); any output or out_null
 * that overlaps an input, an input null or another output / out_null.
 * n_rows == 0 returns GPUE_OK. */
/* leaves */
#define GPUE_X_COL 32
#define GPUE_X_CONST 33
#define GPUE_X_NULL 34
/* unary */
#define GPUE_X_NEG 40
#define GPUE_X_ABS 41
#define GPUE_X_NOT 42
#define GPUE_X_IS_NULL 43
#define GPUE_X_CAST_I32 44
/* binary arithmetic */
#define GPUE_X_ADD 48
#define GPUE_X_SUB 49
#define GPUE_X_MUL 50
#define GPUE_X_DIV 51
#define GPUE_X_MOD 52
/* comparisons */
#define GPUE_X_EQ 56
#define GPUE_X_NE 57
#define GPUE_X_LT 58
#define GPUE_X_LE 59
#define GPUE_X_GT 60
#define GPUE_X_GE 61
/* logic, select, output */
#define GPUE_X_AND 64
#define GPUE_X_OR 65
#define GPUE_X_IF 66
#define GPUE_X_IFNULL 67
#define GPUE_X_OUT 68
/* OR-ed into ADD / SUB / MUL / NEG / ABS: signed overflow -> NULL */
#define GPUE_X_CHECKED 0x200
/* output types */
#define GPUE_XO_I32 0
#define GPUE_XO_I64 1
#define GPUE_XO_MASK 2
#define GPUE_EXPR_MAX_INSNS 64
#define GPUE_EXPR_MAX_STACK 8
#define GPUE_EXPR_MAX_OUT 8
#define GPUE_EXPR_MAX_IN_COLS 64
int gpue_expr_project(gpue_session* s,
                      gpue_dbuf** in_cols,
                      gpue_dbuf** in_nulls, /* may be NULL; entries may be NULL; u8, nonzero = NULL row */
                      const int32_t* in_type /* GPUE_PT_I32 / GPUE_PT_I64 */, int n_in_cols,
                      const int32_t* insn_op, const int32_t* insn_col,
                      const int64_t* insn_a, int n_insns,
                      gpue_dbuf** out_cols,
                      gpue_dbuf** out_nulls, /* may be NULL; entries may be NULL; u8, 1 = NULL row */
                      const int32_t* out_type /* GPUE_XO_I32 / GPUE_XO_I64 / GPUE_XO_MASK */,
                      int n_out, uint64_t n_rows);

/* ---- hash-join build ----
 * Replaces JoinHashTable::build with the RANGE_DIRECT_MAPPING method the
 * selector takes for dense int keys (reference
 * be/src/exec/join/join_hash_table.cpp:263-321,
 * join_hash_map_method.hpp:625-707). Build rows are 1-based; row 0 is the
 * chain-end sentinel (join_hash_table.cpp:590-596).
 *
 * Payload variant (the fused fast path): first[key-min] holds
 * a caller-provided uint32 payload (0 = dim row filtered out / absent). */
typedef struct gpue_join_table gpue_join_table;
int gpue_join_build_payload_i32(gpue_session* s, gpue_dbuf* keys /*i32*/,
                                gpue_dbuf* payloads /*u32*/, uint64_t n_rows,
                                gpue_join_table** out);
/* BUCKET_CHAINED variant — the selector's generic fallback for non-dense
 * keys (join_hash_map_method.hpp:37-120): multiplicative-hash buckets +
 * first/next chains; probe compares build keys along the chain. */
int gpue_join_build_bucket_chained_u32(gpue_session* s, gpue_dbuf* keys /*u32, 1-based*/,
                                       uint64_t row_count, gpue_join_table** out);
/* LINEAR_CHAINED variant — the selector's preferred method under its
 * 16M-bucket cap (join_hash_map_method.h:118-150): 8-bit fingerprint packed
 * in first[], linear probing, same-key chains via next[]. */
int gpue_join_build_linear_chained_u32(gpue_session* s, gpue_dbuf* keys /*u32, 1-based*/,
                                       uint64_t row_count, gpue_join_table** out);
/* 8-byte (BIGINT) key bucket-chained variant — JoinKeyHash<8>
 * (join_hash_map_helper.h:46-55), u64 build-key compares along chains. */
int gpue_join_build_bucket_chained_u64(gpue_session* s, gpue_dbuf* keys /*u64, 1-based*/,
                                       uint64_t row_count, gpue_join_table** out);
/* 16-byte keys (TYPE_LARGEINT / SERIALIZED_FIXED_SIZE_LARGEINT packing):
 * the generic JoinKeyHash<T,16> — crc32 over the key bytes, CRC_SEED,
 * masked by bucket_size-1 (join_hash_map_helper.h:23-30). */
int gpue_join_build_bucket_chained_u128(gpue_session* s, gpue_dbuf* keys /*16 B, 1-based*/,
                                        uint64_t row_count, gpue_join_table** out);
int gpue_join_probe_emit_mode_u128(gpue_session* s, gpue_join_table* t,
                                   gpue_dbuf* probe_keys, uint64_t n_rows, int mode,
                                   gpue_dbuf* out_probe_idx, gpue_dbuf* out_build_idx,
                                   uint64_t* match_count);
int gpue_join_probe_emit_mode_u64(gpue_session* s, gpue_join_table* t, gpue_dbuf* probe_keys,
                                  uint64_t n_rows, int mode, gpue_dbuf* out_probe_idx,
                                  gpue_dbuf* out_build_idx, uint64_t* match_count);
/* Row-index variant: first/next chain structure exactly as the reference
 * builds it (chain order under duplicate keys is scatter-order, which on GPU
 * is nondeterministic — the emitted match multiset is identical). */
int gpue_join_build_range_direct_i32(gpue_session* s, gpue_dbuf* keys /*i32, 1-based row 0 sentinel*/,
                                     uint64_t row_count, gpue_join_table** out);
/* DENSE_RANGE_DIRECT_MAPPING (join_hash_map_method.h:378, .hpp:781-940):
 * rank/select-compressed direct map — per 32-key group a {start_index,
 * bitset} pair (2 bits/interval position amortized), first[] sized by the
 * PRESENT keys; probe = bit test + popcount + one first[] load; chains hold
 * identical keys (no compare). The selector's choice when the interval
 * exceeds bucket/L2 but 2b/pos + 4 B/row beats bucket-chained. */
int gpue_join_build_dense_range_direct_i32(gpue_session* s, gpue_dbuf* keys,
                                           uint64_t row_count, gpue_join_table** out);

/* ---- JoinHashMapSelector (join_hash_table.cpp:164-344) --------------------
 * The reference's automatic key-constructor + map-method decision, restated
 * as pure host functions. Probe-mode values double as the join_type input.
 */
#define GPUE_JOIN_INNER 0
#define GPUE_JOIN_LEFT_SEMI 1
#define GPUE_JOIN_LEFT_ANTI 2
#define GPUE_JOIN_LEFT_OUTER 3
/* key-constructor classes (JoinKeyConstructorUnaryType, :164-229) */
#define GPUE_KEYCON_ONE_KEY 0
#define GPUE_KEYCON_ONE_KEY_VARCHAR 1
#define GPUE_KEYCON_FIXED_INT 2      /* SERIALIZED_FIXED_SIZE_INT, packed <= 4 B */
#define GPUE_KEYCON_FIXED_BIGINT 3   /* packed <= 8 B */
#define GPUE_KEYCON_FIXED_LARGEINT 4 /* packed <= 16 B */
#define GPUE_KEYCON_SERIALIZED_VARCHAR 5
/* map methods (JoinHashMapMethodType, join_hash_map_method.h) */
#define GPUE_JM_DIRECT 0
#define GPUE_JM_RANGE_DIRECT 1
#define GPUE_JM_RANGE_DIRECT_SET 2
#define GPUE_JM_DENSE_RANGE_DIRECT 3
#define GPUE_JM_LINEAR_CHAINED 4
#define GPUE_JM_LINEAR_CHAINED_SET 5
#define GPUE_JM_BUCKET_CHAINED 6
/* logical-type classes for the method decision */
#define GPUE_LT_TINY 0    /* BOOLEAN/TINYINT/SMALLINT -> DIRECT_MAPPING (:239) */
#define GPUE_LT_INT 1
#define GPUE_LT_BIGINT 2
#define GPUE_LT_OTHER 3   /* other fixed-width (largeint/decimal/date...) */
#define GPUE_LT_VARCHAR 4

/* _determine_key_constructor (:164-229). fixed_sizes[i]: key column i's
 * fixed byte width; for varchar keys pass _get_binary_column_max_size's
 * result (1..16 when the fixed-size-string opt applies, else 0).
 * packed_bytes_out: total packed width (0 when not fixed-packed). */
int gpue_join_select_key_constructor(int num_keys, const int32_t* fixed_sizes,
                                     const uint8_t* null_safe,
                                     int enable_fixed_size_string,
                                     int32_t* packed_bytes_out);
/* single-VARCHAR refinement (:178-194) */
int gpue_join_select_varchar_constructor(int32_t max_size, int enable_fixed_size_string);
/* _determine_hash_map_method (:231-256) + range-direct (:270-321) + linear
 * (:323-344) gates. min/max_value: the single int key's bounds over build
 * rows (ignored unless the range-direct gate applies). l2_size/l3_size:
 * reference reads CpuInfo L2 and halves L3 itself (:295-296). Returns a
 * GPUE_JM_* value. */
int gpue_join_select_method(int key_constructor, int lt_class, uint64_t row_count,
                            int64_t min_value, int64_t max_value, int mode,
                            int with_other_conjunct, int enable_range_direct,
                            int enable_linear_chained, uint64_t l2_size,
                            uint64_t l3_size);
/* Auto build for a single i32 key column (keys 1-based, row 0 sentinel):
 * computes the build keys' min/max on device, runs the selector with the
 * reference's default-on session flags, and builds the matching GPU table.
 * l2_size/l3_size 0 -> MI355X defaults (4 MiB XCD L2 / 256 MiB Infinity
 * Cache). method_out (nullable) receives the GPUE_JM_* decision. Mapping to
 * physical layouts: DIRECT/RANGE_DIRECT/RANGE_DIRECT_SET/DENSE map onto the
 * u32 first[] direct-mapped table (the 1-bit SET and 2-bit DENSE packings
 * are CPU-cache idioms; with interval < 2^32 the u32 array is HBM-resident
 * and probes in ONE load — DESIGN.md (S)3), LINEAR_CHAINED(+SET) onto the
 * fp-packed linear-probed table, BUCKET_CHAINED onto first/next chains. */
int gpue_join_build_auto_i32(gpue_session* s, gpue_dbuf* keys, uint64_t row_count,
                             int mode, int with_other_conjunct, uint64_t l2_size,
                             uint64_t l3_size, gpue_join_table** out, int* method_out);
/* 8-byte-key auto build: selector decision with LT_BIGINT reported via
 * method_out; every physical tier maps onto the u64 bucket-chained table
 * (the u64 domain has no range-direct/linear specialization here). */
int gpue_join_build_auto_u64(gpue_session* s, gpue_dbuf* keys, uint64_t row_count,
                             int mode, int with_other_conjunct, uint64_t l2_size,
                             uint64_t l3_size, gpue_join_table** out, int* method_out);
void gpue_join_table_destroy(gpue_join_table* t);
int gpue_join_table_minmax(gpue_join_table* t, int64_t* min_out, int64_t* max_out);
/* d2h the first[] array (tests) */
int gpue_join_table_first_d2h(gpue_join_table* t, uint32_t* dst, uint64_t n_entries);

/* ---- hash-join probe ----
 * Replaces lookup_init + _probe_from_ht chain-walk emit
 * (reference be/src/exec/join/join_hash_map_method.hpp:88-120,
 * join_hash_map.hpp:717-795). Emits all (probe_idx, build_idx) match pairs;
 * out buffers must be sized for the match count (call with out_* NULL to get
 * the count first — the CPU's chunk_size-resumable cursor maps to this
 * two-phase count/emit, SURVEY.md §7 hard part (c)). */
int gpue_join_probe_emit_i32(gpue_session* s, gpue_join_table* t, gpue_dbuf* probe_keys,
                             uint64_t n_rows, gpue_dbuf* out_probe_idx,
                             gpue_dbuf* out_build_idx, uint64_t* match_count);
/* Per-join-type probe (join_hash_map.h:228-333): mode 0 INNER, 1 LEFT_SEMI,
 * 2 LEFT_ANTI (unmatched rows, build index 0 = NULL sentinel), 3 LEFT_OUTER. */
int gpue_join_probe_emit_mode_i32(gpue_session* s, gpue_join_table* t, gpue_dbuf* probe_keys,
                                  uint64_t n_rows, int mode, gpue_dbuf* out_probe_idx,
                                  gpue_dbuf* out_build_idx, uint64_t* match_count);
/* Nullable variants (NullableColumn is_nulls path,
 * join_hash_map_method.hpp:56-120): null build rows never enter a chain;
 * null probe rows match nothing (ANTI/OUTER emit them as unmatched).
 * mode 6 = NULL_AWARE_LEFT_ANTI (the NOT IN lowering, hash_joiner.cpp:97,
 * join_hash_map.hpp:1225-1240): as LEFT_ANTI but null probe rows are
 * EXCLUDED from the output — NULL NOT IN (...) is never true. Also accepted
 * by the varchar nulls probe. */
int gpue_join_build_bucket_chained_nulls_u32(gpue_session* s, gpue_dbuf* keys,
                                             gpue_dbuf* is_nulls /*u8, 1-based*/,
                                             uint64_t row_count, gpue_join_table** out);
int gpue_join_probe_emit_nulls_i32(gpue_session* s, gpue_join_table* t, gpue_dbuf* probe_keys,
                                   gpue_dbuf* probe_nulls /*u8*/, uint64_t n_rows, int mode,
                                   gpue_dbuf* out_probe_idx, gpue_dbuf* out_build_idx,
                                   uint64_t* match_count);
/* Multi-column key packing (SERIALIZED_FIXED_SIZE_BIGINT,
 * join_hash_map_helper.h:112-136): two int32 key columns -> one 8-byte key. */
int gpue_pack_keys_2xi32(gpue_session* s, gpue_dbuf* a, gpue_dbuf* b, uint64_t n,
                         gpue_dbuf* out);
/* two i64 key columns packed into one 16-byte key
 * (SERIALIZED_FIXED_SIZE_LARGEINT, join_key_constructor.h:40-153) */
int gpue_pack_keys_2xi64(gpue_session* s, gpue_dbuf* a, gpue_dbuf* b, uint64_t n,
                         gpue_dbuf* out);
/* SERIALIZED_VARCHAR / Slice keys (the selector's remaining constructor
 * branch, join_hash_map.cpp:269-281 -> JoinKeyHash<Slice>,
 * join_hash_map_helper.h:57-64: crc_hash_32(bytes,len,CRC_HASH_SEED1) masked
 * to the bucket count; probe verifies with a byte compare along the chain).
 * Columns are BinaryColumn-shaped: a bytes buffer + uint32 offsets
 * (binary_column.h:458-459). Build rows are 1-based with row 0 the empty
 * sentinel, so offsets has row_count+2 entries; probe rows are 0-based with
 * n_rows+1 entries. */
int gpue_join_build_varchar(gpue_session* s, gpue_dbuf* bytes, gpue_dbuf* offsets,
                            uint64_t row_count, gpue_join_table** out);
int gpue_join_probe_emit_varchar(gpue_session* s, gpue_join_table* t, gpue_dbuf* pbytes,
                                 gpue_dbuf* poffsets, uint64_t n_rows,
                                 gpue_dbuf* out_probe_idx, gpue_dbuf* out_build_idx,
                                 uint64_t* match_count);
/* Per-join-type Slice probe: mode 0 INNER, 1 LEFT_SEMI, 2 LEFT_ANTI,
 * 3 LEFT_OUTER (join_hash_map.h:228-333 semantics as for the i32 paths). */
int gpue_join_probe_emit_varchar_mode(gpue_session* s, gpue_join_table* t, gpue_dbuf* pbytes,
                                      gpue_dbuf* poffsets, uint64_t n_rows, int mode,
                                      gpue_dbuf* out_probe_idx, gpue_dbuf* out_build_idx,
                                      uint64_t* match_count);
/* Nullable Slice keys (is_nulls semantics as the fixed-size paths:
 * join_hash_map_method.hpp:56-120 — null build rows never chain, null probe
 * rows match nothing; ANTI/OUTER emit them unmatched). is_nulls u8, build
 * side 1-based. */
int gpue_join_build_varchar_nulls(gpue_session* s, gpue_dbuf* bytes, gpue_dbuf* offsets,
                                  gpue_dbuf* is_nulls, uint64_t row_count,
                                  gpue_join_table** out);
int gpue_join_probe_emit_varchar_nulls(gpue_session* s, gpue_join_table* t, gpue_dbuf* pbytes,
                                       gpue_dbuf* poffsets, gpue_dbuf* probe_nulls,
                                       uint64_t n_rows, int mode, gpue_dbuf* out_probe_idx,
                                       gpue_dbuf* out_build_idx, uint64_t* match_count);
/* Accumulating config-2 step: NO per-step accumulator reset — the caller
 * keeps a persistent i64[2] acc and differences successive readbacks.
 * Removes one launch from the 2-op step (SF10 is launch-cost-sensitive). */
int gpue_q1_join_sum_accum(gpue_session* s, gpue_join_table* dates, gpue_dbuf* od,
                           gpue_dbuf* ep, gpue_dbuf* dc, uint64_t n, gpue_dbuf* acc);

typedef struct gpue_agg_table gpue_agg_table; /* defined with the agg section below */

/* ---- streaming pre-aggregation building blocks ----
 * The AUTO-mode streaming agg (aggregate_streaming_sink_operator.cpp:224-310;
 * thresholds aggregator.h:175-178: LowReduction 0.2, HighReduction 0.9,
 * StableLimit 5) over the persistent gpue_agg_table. push = build_hash_map +
 * compute_batch_agg_states (cnts NULL: each row counts 1; non-NULL: rows are
 * pre-aggregated partials, merge_batch semantics aggregate.h:158-168;
 * update_only=1 aggregates only rows whose group exists and marks the rest
 * in miss_mask — the selective pre-agg form); probe_hits =
 * build_hash_map_with_selection's hit count; emit = convert_hash_map_to_chunk.
 * update_only is a FLAGS word: bit 0 = update-only (above); bit 1 =
 * GPUE_AGG_SUM_ONLY — skip the per-row group-count atomic for SUM-only
 * aggregations (the insert leg is atomic-rate bound,
 * profiles/r02_agg_card_ubench.json; a query with no COUNT/AVG function
 * needs no counts and the fused kernels already omit them). Under
 * SUM_ONLY, emit's out_counts for groups touched only by such pushes
 * read 0. */
#define GPUE_AGG_SUM_ONLY 2
int gpue_hash_agg_push_u64(gpue_session* s, gpue_agg_table* at, gpue_dbuf* keys,
                           gpue_dbuf* vals, gpue_dbuf* cnts, uint64_t n, int update_only,
                           gpue_dbuf* miss_mask, uint64_t* hits_out);
int gpue_hash_agg_probe_hits_u64(gpue_session* s, gpue_agg_table* at, gpue_dbuf* keys,
                                 uint64_t n, uint64_t* hits_out);
int gpue_hash_agg_emit_u64(gpue_session* s, gpue_agg_table* at, gpue_dbuf* out_keys,
                           gpue_dbuf* out_sums, gpue_dbuf* out_counts, uint64_t max_out,
                           uint64_t* n_groups);

/* Dictionary-encoded binary page decode (binary_dict_page.cpp:229-280): the
 * data page's int32 codewords (bitshuffle layer via
 * gpue_page_decode_bshuf_lz4_i32) index the dict page's distinct strings
 * (binary_plain_page.h string_at_index); output is a BinaryColumn (bytes +
 * uint32 offsets, 0-based rows). Call with out_* NULL for the byte count. */
int gpue_dict_decode_binary(gpue_session* s, gpue_dbuf* dict_bytes, gpue_dbuf* dict_offsets,
                            gpue_dbuf* codes, uint64_t n, gpue_dbuf* out_bytes,
                            gpue_dbuf* out_offsets, uint64_t* total_bytes);

/* ---- SimdBlockFilter runtime filter ----
 * The reference's split-block bloom (runtime_filter.h:79-232, upstream
 * fastfilter_cpp): 32-byte buckets of 8 uint32 lanes, one bit per lane from
 * (key*SALT[i])>>27; inserted hash = phmap_mix<8>(value) for integer keys
 * (runtime_filter.h:1271-1276). directory must hold 32<<log_num_buckets
 * bytes, where log_num_buckets = max(1, ceil(log2(n))-5)
 * (runtime_filter.cpp:26-36). Build is atomicOr — the directory is
 * bit-identical to the reference's serial build. test writes one u8 per row
 * (1 = maybe-member): the scan-side early prune pushed to probe operators
 * (operator.h:188-199). */
int gpue_sbf_build_i32(gpue_session* s, gpue_dbuf* keys, uint64_t n,
                       int32_t log_num_buckets, gpue_dbuf* directory);
int gpue_sbf_test_i32(gpue_session* s, gpue_dbuf* keys, uint64_t n, gpue_dbuf* directory,
                      int32_t log_num_buckets, gpue_dbuf* out);
/* RIGHT SEMI (anti=0) / RIGHT ANTI (anti=1) over Slice keys. */
int gpue_join_probe_right_varchar(gpue_session* s, gpue_join_table* t, gpue_dbuf* pbytes,
                                  gpue_dbuf* poffsets, uint64_t n_rows, int anti,
                                  gpue_dbuf* out_build_idx, uint64_t* count);
/* RIGHT SEMI (anti=0) / RIGHT ANTI (anti=1): matched/unmatched BUILD rows. */
int gpue_join_probe_right_i32(gpue_session* s, gpue_join_table* t, gpue_dbuf* probe_keys,
                              uint64_t n_rows, int anti, gpue_dbuf* out_build_idx,
                              uint64_t* count);

/* ---- fused probe + aggregate pipelines ----
 * Replace the probe -> output gather -> Aggregator::update_batch chain
 * (reference be/src/exec/join/join_hash_map.hpp:284-330,
 * be/src/exec/aggregator.cpp:937-959, be/src/exprs/agg/sum.h:45-181) with one
 * fused kernel per BASELINE config. Sums are int64, order-independent =>
 * bit-exact vs the oracle. */
/* Config 2 (SSB SF10 Q1-shaped): SUM(lo_extendedprice*lo_discount) over rows
 * whose lo_orderdate matches the (pre-filtered) date dim payload table. */
int gpue_q1_join_sum(gpue_session* s, gpue_join_table* dates, gpue_dbuf* lo_orderdate,
                     gpue_dbuf* lo_extendedprice, gpue_dbuf* lo_discount, uint64_t n_rows,
                     int64_t* sum_out, uint64_t* match_count_out);
/* Async bench variant: zero + launch into a caller-owned 16-byte accumulator
 * ({int64 sum, uint64 count}); no sync, no transient allocation. */
int gpue_q1_join_sum_async(gpue_session* s, gpue_join_table* dates, gpue_dbuf* lo_orderdate,
                           gpue_dbuf* lo_extendedprice, gpue_dbuf* lo_discount,
                           uint64_t n_rows, gpue_dbuf* acc);
/* Config 3 (SSB SF100 Q2.1-shaped): 3-way star probe + GROUP BY
 * (d_year,p_brand) -> dense group id (year_idx*1000+brand), SUM(lo_revenue).
 * group_sums_out must hold 7000 int64. */
int gpue_q21_star_agg(gpue_session* s, gpue_join_table* parts, gpue_join_table* supps,
                      gpue_join_table* dates, gpue_dbuf* lo_partkey, gpue_dbuf* lo_suppkey,
                      gpue_dbuf* lo_orderdate, gpue_dbuf* lo_revenue, uint64_t n_rows,
                      int64_t* group_sums_out);

/* Two-stream pipelined variant: K_A (part runtime-filter probe + brand
 * payload -> u16 per row, brand_scratch) overlaps K_B (remaining streams +
 * supplier/date probes + group agg) across n_chunks chunks — the two legs
 * measured fully additive inside one kernel.
 * Rows are split into n_chunks chunks of ceil(n_rows / n_chunks) rows rounded
 * up to a multiple of 4; trailing empty chunks launch nothing and n_rows == 0
 * returns zeros. brand_scratch is written on the session's second stream
 * while the session stream still reads it, and it is reused across calls:
 * the caller must gpue_sync() before passing the same brand_scratch to a
 * second pipe call (or freeing it). */
int gpue_q21_star_agg_pipe(gpue_session* s, gpue_join_table* parts, gpue_join_table* supps,
                           gpue_join_table* dates, gpue_dbuf* lo_partkey, gpue_dbuf* lo_suppkey,
                           gpue_dbuf* lo_orderdate, gpue_dbuf* lo_revenue, uint64_t n_rows,
                           gpue_dbuf* brand_scratch /* n_rows × u16 */, gpue_dbuf* group_sums,
                           int n_chunks);
/* Async bench variant of the star aggregate (7000 × int64 device buffer). */
int gpue_q21_star_agg_async(gpue_session* s, gpue_join_table* parts, gpue_join_table* supps,
                            gpue_join_table* dates, gpue_dbuf* lo_partkey, gpue_dbuf* lo_suppkey,
                            gpue_dbuf* lo_orderdate, gpue_dbuf* lo_revenue, uint64_t n_rows,
                            gpue_dbuf* group_sums);

/* Config 4 (SSB Q4.3): 4-way star join + GROUP BY (d_year,s_city,p_brand) as
 * compact filtered indexes -> 800 groups; SUM(lo_revenue - lo_supplycost).
 * group_sums holds 800 x int64 on device. */
int gpue_q43_star_agg_async(gpue_session* s, gpue_join_table* custs, gpue_join_table* supps,
                            gpue_join_table* parts, gpue_join_table* dates,
                            gpue_dbuf* lo_custkey, gpue_dbuf* lo_suppkey,
                            gpue_dbuf* lo_partkey, gpue_dbuf* lo_orderdate,
                            gpue_dbuf* lo_revenue, gpue_dbuf* lo_supplycost,
                            uint64_t n_rows, gpue_dbuf* group_sums);

/* ---- exchange partition (shuffle groundwork for configs 4-5) ----
 * Replaces the ExchangeSinkOperator partition stage
 * (reference be/src/exec/pipeline/exchange/exchange_sink_operator.cpp:611-660,
 * shuffler.h:71-86): per-row FNV hash -> ReduceOp channel -> counting-sort
 * row layout, bit-identical to the reference's (stable: each channel's rows
 * ascend by source row). start_points has num_channels+1 entries. */
/* Version-1 exchange hash (xxh3) partition — the
 * `_exchange_hash_function_version == 1` branch of
 * exchange_sink_operator.cpp:604-610 (XXH3_64bits_withSeed per key value,
 * seed XXH3_SEED_32, truncated u32; restated from the published XXH3 spec
 * and pinned to python-xxhash vectors in tests/golden/xxh3_kats.json).
 * FNV (gpue_partition_i32) stays the reference's backward-compatible
 * default. */
int gpue_partition_xxh3_i32(gpue_session* s, gpue_dbuf* keys, uint64_t n,
                            uint32_t num_channels, uint64_t* start_points_out,
                            gpue_dbuf* row_indexes_out);
/* The bucket-shuffle hash path (zlib crc32, seed 0 — the third of the
 * exchange's three hash functions, exchange_sink_operator.cpp:617-622;
 * pinned live against python zlib). */
int gpue_partition_crc_i32(gpue_session* s, gpue_dbuf* keys, uint64_t n,
                           uint32_t num_channels, uint64_t* start_points_out,
                           gpue_dbuf* row_indexes_out);
/* Varchar (BinaryColumn) partition key: FNV over the slice bytes. */
int gpue_partition_varchar(gpue_session* s, gpue_dbuf* bytes, gpue_dbuf* offsets,
                           uint64_t n, uint32_t num_channels,
                           uint64_t* start_points_out, gpue_dbuf* row_indexes_out);
/* Steady-state async partition: hist -> DEVICE-side scan -> emit with no
 * host round-trip (the sync forms host-scan the histogram to return split
 * sizes; in the chunked exchange the splits are static per shard, so the
 * timed step only needs row_indexes). scratch holds the per-(block,channel)
 * histogram + offsets (>= grid*channels*12 bytes). */
int gpue_partition_i32_async(gpue_session* s, gpue_dbuf* keys, uint64_t n,
                             uint32_t num_channels, gpue_dbuf* row_indexes_out,
                             gpue_dbuf* scratch);
int gpue_partition_i64_async(gpue_session* s, gpue_dbuf* keys, uint64_t n,
                             uint32_t num_channels, gpue_dbuf* row_indexes_out,
                             gpue_dbuf* scratch);
int gpue_partition_i32(gpue_session* s, gpue_dbuf* keys, uint64_t n, uint32_t num_channels,
                       uint64_t* start_points_out, gpue_dbuf* row_indexes_out);
/* Multi-column partition key: the sink seeds FNV_SEED then CHAINS fnv_hash
 * per partition column, each column seeding with the running hash
 * (exchange_sink_operator.cpp:611-617). Two-int32-column variant. */
int gpue_partition_2xi32(gpue_session* s, gpue_dbuf* a, gpue_dbuf* b, uint64_t n,
                         uint32_t num_channels, uint64_t* start_points_out,
                         gpue_dbuf* row_indexes_out);

/* ---- config 5: TPC-H Q3-shaped ----
 * lineitem ⋈ orders ⋈ customer; c_mktsegment = 16-byte dictionary string
 * (SERIALIZED_FIXED_SIZE_LARGEINT packing, join_hash_table.cpp:185-192);
 * revenue = extendedprice(cents) × (100−discount), scale-4 decimal int64;
 * GROUP BY l_orderkey (high cardinality) via the hash aggregate below. */
int gpue_gen_lineitem_q3(gpue_session* s, uint64_t seed, uint64_t row_start, uint64_t n,
                         uint64_t n_orders, gpue_dbuf* l_orderkey /*i64*/,
                         gpue_dbuf* l_extendedprice /*i64*/, gpue_dbuf* l_discount /*i64*/,
                         gpue_dbuf* l_shipdate /*i32*/);
int gpue_gen_orders_q3(gpue_session* s, uint64_t seed, uint64_t n_orders, uint32_t n_custs,
                       gpue_dbuf* o_custkey, gpue_dbuf* o_orderdate);
int gpue_gen_cust_mkt16(gpue_session* s, uint64_t seed, uint32_t n_custs, gpue_dbuf* out);
/* 16-byte fixed-string equality -> membership bitset (two u64 compares) */
int gpue_bits_str16_eq(gpue_session* s, gpue_dbuf* col16, uint64_t n, const void* lit16,
                       gpue_dbuf* bits);
/* orders pass bitset: o_orderdate < cutoff AND customer bit set */
int gpue_q3_order_bits(gpue_session* s, gpue_dbuf* o_custkey, gpue_dbuf* o_orderdate,
                       uint64_t n_orders, gpue_dbuf* cust_bits, int32_t cutoff,
                       gpue_dbuf* order_bits);
/* persistent aggregate table (per-query hash map analog, reused across
 * passes so repeated executions pay reset, not allocation) */
int gpue_agg_table_create(gpue_session* s, uint64_t capacity, gpue_agg_table** out);
void gpue_agg_table_destroy(gpue_agg_table* t);
/* fused lineitem filter + orders semi-probe + hash aggregate */
int gpue_q3_probe_agg(gpue_session* s, gpue_dbuf* lk, gpue_dbuf* ext, gpue_dbuf* disc,
                      gpue_dbuf* ship, uint64_t n, gpue_dbuf* order_bits, int32_t ship_cutoff,
                      uint64_t capacity_hint, gpue_dbuf* out_keys, gpue_dbuf* out_sums,
                      uint64_t max_out, uint64_t* n_groups);
/* variant over a persistent gpue_agg_table (reset + probe + emit) */
int gpue_q3_probe_agg_t(gpue_session* s, gpue_dbuf* lk, gpue_dbuf* ext, gpue_dbuf* disc,
                        gpue_dbuf* ship, uint64_t n, gpue_dbuf* order_bits,
                        int32_t ship_cutoff, gpue_agg_table* at, gpue_dbuf* out_keys,
                        gpue_dbuf* out_sums, uint64_t max_out, uint64_t* n_groups);

/* ---- generic hash aggregate ----
 * Replaces AggHashMapWithKey::compute_agg_states + update_batch +
 * convert_hash_map_to_chunk (reference be/src/exec/agg_hash_map.h:112-290,
 * aggregator.cpp:937-959,1742-1816) for HIGH-cardinality GROUP BY (group-key
 * packed <= 8 B, as the SERIALIZED_FIXED_SIZE key constructors pack). SUM +
 * COUNT states; emission order is table order (results are a set). Key
 * sentinel ~0ull must not occur in keys. */
int gpue_hash_agg_sum_u64(gpue_session* s, gpue_dbuf* keys /*u64*/, gpue_dbuf* vals /*i64*/,
                          uint64_t n, uint64_t capacity_hint, gpue_dbuf* out_keys,
                          gpue_dbuf* out_sums, gpue_dbuf* out_counts /*nullable*/,
                          uint64_t max_out, uint64_t* n_groups);

/* Full aggregate-function states: SUM + COUNT + MIN + MAX (AVG = SUM/COUNT
 * at finalize, reference exprs/agg/aggregate.h:136-269). */
int gpue_hash_agg_stats_u64(gpue_session* s, gpue_dbuf* keys, gpue_dbuf* vals, uint64_t n,
                            uint64_t capacity_hint, gpue_dbuf* out_keys, gpue_dbuf* out_sums,
                            gpue_dbuf* out_counts, gpue_dbuf* out_mins, gpue_dbuf* out_maxs,
                            uint64_t max_out, uint64_t* n_groups);
/* Decimal SUM widened to int128 (exprs/agg/sum.h:181): lo/hi pair with an
 * explicit carry, exact mod 2^128, order-independent. */
int gpue_hash_agg_sum128_u64(gpue_session* s, gpue_dbuf* keys, gpue_dbuf* vals, uint64_t n,
                             uint64_t capacity_hint, gpue_dbuf* out_keys, gpue_dbuf* out_lo,
                             gpue_dbuf* out_hi, uint64_t max_out, uint64_t* n_groups);

/* Row gather by index — the exchange sink's add_rows_selective analog
 * (exchange_sink_operator.cpp:670): materializes per-channel row slices at
 * the counting-sorted indexes before the RCCL all-to-all. */
int gpue_gather_u32(gpue_session* s, gpue_dbuf* in, gpue_dbuf* idx, uint64_t n,
                    gpue_dbuf* out);
int gpue_gather_u64(gpue_session* s, gpue_dbuf* in, gpue_dbuf* idx, uint64_t n,
                    gpue_dbuf* out);
/* 1-byte form of the same gather (Column::append_selective over a
 * NullColumn's u8 data): carries null masks behind a sort permutation. */
int gpue_gather_u8(gpue_session* s, gpue_dbuf* in, gpue_dbuf* idx, uint64_t n,
                   gpue_dbuf* out);
/* BIGINT-key partition (FNV over the 8 LE bytes of an int64 key column) */
int gpue_partition_i64(gpue_session* s, gpue_dbuf* keys, uint64_t n, uint32_t num_channels,
                       uint64_t* start_points_out, gpue_dbuf* row_indexes_out);

/* ---- storage ingress (the step upstream of the scan) ----
 * Decode the reference's numeric page body (bitshuffle+LZ4,
 * be/src/storage/rowset/bitshuffle_page.h framing after the 16-byte header;
 * bitshuffle 0.5.1 published algorithm + LZ4 block format restated in
 * oracle/oracle.c): n_values int32 (multiple of 8) from the device-resident
 * page bytes. */
int gpue_page_decode_bshuf_lz4_i32(gpue_session* s, gpue_dbuf* page, uint32_t n_values,
                                   gpue_dbuf* out);

/* ---- TopN ----
 * ORDER BY value DESC LIMIT k (reference exec/chunks_sorter_topn.cpp):
 * deterministic (value, key) lexicographic descending; k <= 16. */
int gpue_topk_i64(gpue_session* s, gpue_dbuf* keys, gpue_dbuf* vals, uint64_t n,
                  int k, uint64_t* out_keys, int64_t* out_vals);
/* General TopN: multi-key ORDER BY ... LIMIT/OFFSET for any k — the
 * ChunksSorterTopn result (reference exec/chunks_sorter_topn.cpp) under the
 * reference's SortDesc (per-key sort direction + null placement,
 * exec/sorting/sorting.h SortDesc/SortDescs). Output = positions
 * [offset, offset+limit) of the total order of all n_rows rows, as u32 row
 * indices in result order; out_count = min(limit, max(n_rows - offset, 0)).
 * Order: lexicographic over the keys, each ascending or descending by its
 * flag; a NULL row sorts before every non-NULL value of that key under
 * NULLS_FIRST, after under NULLS_LAST, whatever the direction; the stored
 * value of a NULL row is never read into the order. Rows equal on every key
 * (two NULLs of one key included) come out in ascending row index — the
 * reference leaves that order unspecified; pinning it makes the result equal
 * a stable sort. Payload columns are materialized by the caller with
 * gpue_gather_u32/u64 over out_row_idx. GPUE_ERR_ARG (before any launch)
 * for n_keys outside 1..8, an unknown key type, n_rows >= 2^32, a key/null
 * buffer shorter than n_rows elements, or out_row_idx shorter than
 * out_count*4 bytes; n_rows == 0, limit == 0 and offset >= n_rows return
 * GPUE_OK with count 0. key_nulls may itself be NULL (no nullable key). */
#define GPUE_TOPN_I32 0
#define GPUE_TOPN_I64 1
#define GPUE_TOPN_U64 2
#define GPUE_TOPN_DESC 1        /* key_flags bit 0 */
#define GPUE_TOPN_NULLS_FIRST 2 /* key_flags bit 1 */
int gpue_topn(gpue_session* s,
              gpue_dbuf** key_cols,      /* n_keys sort columns, most significant first */
              gpue_dbuf** key_nulls,     /* n_keys entries; each NULL or a u8 mask, nonzero = NULL row */
              const int32_t* key_type,   /* GPUE_TOPN_I32 / _I64 / _U64 */
              const int32_t* key_flags,  /* GPUE_TOPN_DESC | GPUE_TOPN_NULLS_FIRST */
              int n_keys, uint64_t n_rows,
              uint64_t offset, uint64_t limit,
              gpue_dbuf* out_row_idx,    /* u32 row indices, in result order */
              uint64_t* out_count);
/* Full sort: multi-key ORDER BY without LIMIT — the ChunksSorterFullSort
 * result (reference exec/chunks_sorter_full_sort.cpp) under the same SortDesc
 * as gpue_topn. out_row_idx receives the whole order, bit-identical to what
 * gpue_topn writes for the same keys with offset = 0, limit = n_rows:
 * lexicographic under each key's direction, NULL placement independent of the
 * direction, the cell under a NULL never read into the order, rows equal on
 * every key in ascending row index. Same key arguments and the same
 * GPUE_ERR_ARG cases (before any launch or allocation) as gpue_topn, with
 * out_row_idx at least n_rows*4 bytes; n_rows == 0 returns GPUE_OK with
 * nothing written. Device side: a stable LSD radix sort (8-bit digits) over
 * only the digits on which a key varies; up to GPUE_SORT_SMALL_MAX rows it
 * runs gpue_topn's single-tile path instead. Workspace is allocated per call
 * and freed on every path: at most 20 bytes per row (a second u32 row buffer
 * and two 8-byte key-image buffers; 12 with only int32 keys) plus 1 MiB of
 * block histograms. Payload columns are materialized by the caller with
 * gpue_gather_u8/u32/u64 over out_row_idx. */
#define GPUE_SORT_SMALL_MAX 2048
int gpue_sort(gpue_session* s,
              gpue_dbuf** key_cols, gpue_dbuf** key_nulls,
              const int32_t* key_type,   /* GPUE_TOPN_I32 / _I64 / _U64 */
              const int32_t* key_flags,  /* GPUE_TOPN_DESC | GPUE_TOPN_NULLS_FIRST */
              int n_keys, uint64_t n_rows,
              gpue_dbuf* out_row_idx);   /* u32[n_rows]: the whole order */

/* ---- chunked-exchange overlap support (SURVEY.md §7 hard part (d)) ------
 * The session's HIP stream as an opaque pointer (wrap as a torch
 * ExternalStream to event-order RCCL collectives against engine kernels),
 * plus accumulate-only forms of the probe+agg steps so a received row-block
 * can be probed while the next block's all-to-all is in flight — the analog
 * of the reference's overlapped SinkBuffer (sink_buffer.cpp:533-536). */
void* gpue_session_stream(gpue_session* s);
int gpue_q43_star_agg_accum_async(gpue_session* s, gpue_join_table* custs,
                                  gpue_join_table* supps, gpue_join_table* parts,
                                  gpue_join_table* dates, gpue_dbuf* ck, gpue_dbuf* sk,
                                  gpue_dbuf* pk, gpue_dbuf* od, gpue_dbuf* rv,
                                  gpue_dbuf* sc, uint64_t n, gpue_dbuf* group_sums);
int gpue_q3_probe_accum(gpue_session* s, gpue_dbuf* lk, gpue_dbuf* ext, gpue_dbuf* disc,
                        gpue_dbuf* ship, uint64_t n, gpue_dbuf* order_bits,
                        int32_t ship_cutoff, gpue_agg_table* at);

/* ---- growable agg table ----
 * The MI355X analog of the reference's two-level conversion
 * (Aggregator::try_convert_to_two_level_map, aggregator.cpp:1237-1241;
 * agg_hash_variant.cpp:318): size() reads the claimed-group counter;
 * ensure() doubles + rehashes on device until a push of additional_rows can
 * never overflow (load factor kept <= 5/8). Call before each chunk push,
 * as the reference checks before each chunk. */
int gpue_agg_table_size(gpue_session* s, gpue_agg_table* t, uint64_t* n_groups);
int gpue_agg_table_ensure(gpue_session* s, gpue_agg_table* t, uint64_t additional_rows);

/* ---- general GROUP BY: multi-key, multi-aggregate, NULL-aware -----------
 * The whole AggHashMapWithKey::compute_agg_states + update_batch /
 * merge_batch + convert_hash_map_to_chunk chain (reference agg_hash_map.h,
 * aggregator.cpp, exprs/agg/aggregate.h) behind one persistent, growable
 * table whose key / aggregate layout is fixed at creation. It takes the
 * nullable column format gpue_pred_eval_mask and gpue_expr_project produce:
 * a value column plus a u8 null column.
 *
 * Keys: 1..GPUE_GA_MAX_KEYS columns, GPUE_PT_I32 (sign-extended) or
 * GPUE_PT_I64. Every 64-bit pattern is a legal key value, ~0 included (the
 * table has no key sentinel). A row is NULL on key i iff key_nulls[i][row]
 * is nonzero. NULL equals NULL for grouping, and the value stored under a
 * NULL key is never read: rows that are NULL on key i and equal elsewhere
 * are one group whatever sits in their value cells. key_nulls (or an entry)
 * may be NULL for a key declared nullable — no NULLs in this chunk; a
 * non-NULL null buffer for a key declared non-nullable is GPUE_ERR_ARG.
 *
 * Aggregates: 0..GPUE_GA_MAX_AGGS (0 = DISTINCT). COUNT_STAR counts rows and
 * takes no input column; COUNT counts non-NULL inputs; SUM (wrapping mod
 * 2^64, as gpue_hash_agg_sum_u64), MIN and MAX ignore NULL inputs. The same
 * rule as for keys holds for agg_nulls. Output nullability is static:
 * COUNT_STAR and COUNT never; SUM / MIN / MAX iff their input was declared
 * nullable, and a group that saw no non-NULL input emits NULL (value 0, null
 * byte 1). All aggregate outputs are int64.
 *
 * GPUE_GA_MERGE (push flag): the inputs are partial states as emit produces
 * them — every aggregate input is an int64 column, COUNT_STAR has one too,
 * COUNT / COUNT_STAR add their input, SUM / MIN / MAX combine as usual, a
 * NULL partial is skipped (merge_batch; what the cnts argument of
 * gpue_hash_agg_push_u64 covers for one column).
 *
 * emit: keys in their own types (0 under NULL) with u8 1/0 null columns for
 * nullable keys (out_key_nulls entries of non-nullable keys are ignored),
 * then the aggregates with null columns for nullable outputs. Order is table
 * order; results are a set, compare key-sorted. The table stays intact: push
 * -> emit -> push -> emit is legal. More groups than max_out: GPUE_ERR_ARG
 * with *n_groups set to the true count, nothing written.
 *
 * Never full: push works in sub-batches of at most 2^20 rows and, before
 * each, doubles + rehashes on device until load <= 5/8 even if every row of
 * the sub-batch were a new group (the gpue_agg_table_ensure rule);
 * capacity_hint is only a starting size. No lane ever waits on another
 * lane's store: every loop is a probe walk bounded by the capacity
 * (DESIGN.md §4g).
 *
 * GPUE_ERR_ARG, before any launch or allocation, for: n_keys outside
 * 1..GPUE_GA_MAX_KEYS, n_aggs outside 0..GPUE_GA_MAX_AGGS, an unknown type,
 * function or flag, n_rows >= 2^32, any buffer shorter than n_rows (or
 * max_out) elements, a missing input or output column (a nullable output
 * needs its null column), an output that overlaps another output.
 * n_rows == 0 returns GPUE_OK. No GROUP BY at all (n_keys == 0) and int128
 * sums are not covered: gpue_hash_agg_sum128_u64 stays the int128 entry. */
typedef struct gpue_group_agg gpue_group_agg;
#define GPUE_GA_MAX_KEYS 4
#define GPUE_GA_MAX_AGGS 8
#define GPUE_GA_COUNT_STAR 0   /* no input column in normal mode */
#define GPUE_GA_COUNT 1        /* COUNT(col): non-NULL rows */
#define GPUE_GA_SUM 2          /* int64, wrapping mod 2^64 like the existing SUM */
#define GPUE_GA_MIN 3
#define GPUE_GA_MAX 4
#define GPUE_GA_MERGE 1        /* push flag: inputs are partial states */
int gpue_group_agg_create(gpue_session* s, const int32_t* key_type /* GPUE_PT_I32 / _I64 */,
                          const int32_t* key_nullable, int n_keys,
                          const int32_t* agg_fn,
                          const int32_t* agg_type /* GPUE_PT_*; ignored for COUNT_STAR */,
                          const int32_t* agg_nullable, int n_aggs /* 0..8; 0 = DISTINCT */,
                          uint64_t capacity_hint, gpue_group_agg** out);
int gpue_group_agg_push(gpue_session* s, gpue_group_agg* t, gpue_dbuf** key_cols,
                        gpue_dbuf** key_nulls, gpue_dbuf** agg_cols, gpue_dbuf** agg_nulls,
                        uint64_t n_rows, int flags);
int gpue_group_agg_size(gpue_session* s, gpue_group_agg* t, uint64_t* n_groups);
int gpue_group_agg_emit(gpue_session* s, gpue_group_agg* t, gpue_dbuf** out_keys,
                        gpue_dbuf** out_key_nulls, gpue_dbuf** out_aggs,
                        gpue_dbuf** out_agg_nulls, uint64_t max_out, uint64_t* n_groups);
int gpue_group_agg_reset(gpue_group_agg* t);
void gpue_group_agg_destroy(gpue_group_agg* t);

/* ---- general hash join: multi-key, NULL-aware, every join type ----------
 * One persistent, growable join table beside the per-key-shape entries above
 * (gpue_join_build_* / gpue_join_probe_emit_*, which stay as they are). It
 * restates join_hash_map.h:228-333 (the per-join-type probes),
 * join_hash_map_method.hpp (build and lookup) and join_key_constructor.h
 * (multi-key handling: here the tuple is compared column by column instead of
 * being serialised), and takes the nullable column format gpue_expr_project
 * and gpue_group_agg_emit produce: a value column plus a u8 null column.
 * Everything is exact (integers only).
 *
 * Keys: 1..GPUE_HJ_MAX_KEYS columns, each GPUE_PT_I32 or GPUE_PT_I64,
 * declared separately for the build and the probe side. Values compare as
 * sign-extended int64, so an int32 foreign key joins an int64 primary key.
 * Every 64-bit pattern is a legal key; there is no sentinel. The null rules
 * are those of gpue_group_agg_push: key_nulls (or an entry) may be NULL for a
 * key declared nullable — no NULLs in this chunk; a non-NULL null buffer for
 * a key declared non-nullable is GPUE_ERR_ARG; the cell under a NULL is never
 * read into a hash or a compare. key_nullable covers both sides.
 *
 * Equality: a row that is NULL on a key with key_null_safe[i] == 0 matches
 * nothing. With key_null_safe[i] == 1 (the <=> operator) NULL equals NULL and
 * nothing else on that key. A build row that can match nothing is still a
 * build row: it has an index, is never marked, and emit_build(matched = 0)
 * reports it.
 *
 * Build: build_push may be called any number of times; build rows are
 * numbered FROM 0 in push order across pushes (unlike the 1-based rows of the
 * old entries). The table copies the keys, so the pushed buffers may be freed
 * when the call returns. The table never fills: capacity_hint is a starting
 * size, and before a push the slot array doubles on the device until load
 * <= 5/8 even if every pushed row were a new tuple, re-inserting the occupied
 * slots from the table's own key store (no host round trip over rows).
 * n_rows == 0 is GPUE_OK. Total build rows stay below 2^32-1 (more is
 * GPUE_ERR_ARG). A build_push after a probe is legal; existing marks persist.
 * gpue_hash_join_stats reports {slot capacity, distinct matchable tuples,
 * doublings of the slot array so far, re-insert passes so far}.
 *
 * Probe: emits (probe_idx, build_idx) as two u32 columns; probe_idx is
 * relative to this call, build_idx is the global build row. Both outputs
 * NULL: *count only (the count-then-emit protocol of the old entries). An
 * output shorter than *count elements is GPUE_ERR_ARG, *count is set and
 * nothing is written. out_probe_idx is non-decreasing; the order of one probe
 * row's matches is unspecified.
 *   INNER       every match
 *   LEFT_SEMI   one pair per probe row with a match; which of its matches is
 *               unspecified
 *   LEFT_ANTI   (i, NO_ROW) per probe row without a match, rows with a NULL
 *               key included
 *   LEFT_OUTER  INNER plus (i, NO_ROW) for unmatched rows
 *   NULL_AWARE_LEFT_ANTI  SQL NOT IN: over an empty build every probe row is
 *               emitted, NULL ones too; else, if any build row has a NULL
 *               key, nothing; else LEFT_ANTI without the NULL probe rows.
 *               n_keys == 1 and a non-null-safe key only (else GPUE_ERR_ARG).
 *               This differs on purpose from mode 6 of the old entries.
 *   MARK_ONLY   emits nothing (*count = 0, outputs ignored), implies
 *               GPUE_HJ_MARK_BUILD
 * With GPUE_HJ_MARK_BUILD every build row that matched some probe row is
 * marked in a bitmap the table keeps across probe calls (reset_marks clears
 * it). A call takes at most 2^32-1 probe rows and one probe row at most
 * 2^32-1 matches.
 *
 * RIGHT and FULL are compositions:
 *   RIGHT OUTER  INNER probes with MARK_BUILD, then emit_build(matched = 0)
 *   FULL OUTER   LEFT_OUTER probes with MARK_BUILD, then emit_build(0)
 *   RIGHT SEMI   MARK_ONLY probes, then emit_build(1)
 *   RIGHT ANTI   MARK_ONLY probes, then emit_build(0)
 *
 * emit_build writes the selected build rows in ascending index order. More
 * than max_out of them: GPUE_ERR_ARG with *count the true count and nothing
 * written. out NULL: *count only.
 *
 * gpue_gather_outer materialises a payload column through an index column
 * that may hold NO_ROW: idx[j] == NO_ROW gives out[j] = 0, out_nulls[j] = 1;
 * otherwise out[j] = in[idx[j]] and out_nulls[j] = in_nulls[idx[j]] (0 when
 * in_nulls is NULL). width is the element size, 1, 4 or 8. out_nulls may be
 * NULL only when the caller knows there is no NO_ROW and passes no in_nulls:
 * a NO_ROW met without out_nulls is GPUE_ERR_ARG, and so is any other index
 * >= in_rows — both reported through a device-side latch after the kernel,
 * never by a fault (the rule gpue_window_eval states for order_idx); the
 * outputs are then unspecified.
 *
 * GPUE_ERR_ARG, before any launch or allocation, for: n_keys outside
 * 1..GPUE_HJ_MAX_KEYS, an unknown type, mode or flag, n_rows >= 2^32, a
 * buffer shorter than n_rows (or max_out) elements, a missing key column,
 * only one of the two probe outputs, outputs that overlap each other or an
 * input.
 *
 * No lane waits on another lane's store: every device loop is a slot walk
 * bounded by the capacity or a chain walk bounded by the tuple's row count,
 * and a bound that is hit latches GPUE_ERR_HIP.
 *
 * Not covered: residual ("other") conjuncts evaluated inside the probe —
 * filter the emitted pairs; varchar / float / decimal128 keys (the varchar
 * entries above stay the route); more than 2^32-1 build rows; spilling. */
typedef struct gpue_hash_join gpue_hash_join;
#define GPUE_HJ_MAX_KEYS 4
#define GPUE_HJ_NO_ROW 0xFFFFFFFFu      /* "no row on this side" in an index column */
/* probe modes */
#define GPUE_HJ_INNER 0
#define GPUE_HJ_LEFT_SEMI 1
#define GPUE_HJ_LEFT_ANTI 2
#define GPUE_HJ_LEFT_OUTER 3
#define GPUE_HJ_NULL_AWARE_LEFT_ANTI 4  /* NOT IN; n_keys == 1 only */
#define GPUE_HJ_MARK_ONLY 5             /* emits nothing; implies GPUE_HJ_MARK_BUILD */
/* probe flag */
#define GPUE_HJ_MARK_BUILD 1            /* also mark every matched build row */
int gpue_hash_join_create(gpue_session* s, const int32_t* build_key_type,
                          const int32_t* probe_key_type, const int32_t* key_nullable,
                          const int32_t* key_null_safe, int n_keys, uint64_t capacity_hint,
                          gpue_hash_join** out);
int gpue_hash_join_build_push(gpue_session* s, gpue_hash_join* t, gpue_dbuf** key_cols,
                              gpue_dbuf** key_nulls, uint64_t n_rows);
int gpue_hash_join_build_rows(gpue_hash_join* t, uint64_t* n_rows);
int gpue_hash_join_stats(gpue_hash_join* t, uint64_t* out4);
int gpue_hash_join_probe(gpue_session* s, gpue_hash_join* t, gpue_dbuf** key_cols,
                         gpue_dbuf** key_nulls, uint64_t n_rows, int mode, int flags,
                         gpue_dbuf* out_probe_idx, gpue_dbuf* out_build_idx, uint64_t* count);
int gpue_hash_join_emit_build(gpue_session* s, gpue_hash_join* t, int matched /* 1 or 0 */,
                              gpue_dbuf* out_build_idx, uint64_t max_out, uint64_t* count);
int gpue_hash_join_reset_marks(gpue_session* s, gpue_hash_join* t);
void gpue_hash_join_destroy(gpue_hash_join* t);
int gpue_gather_outer(gpue_session* s, gpue_dbuf* in, gpue_dbuf* in_nulls /* or NULL */,
                      uint64_t in_rows, int width /* 1, 4, 8 */, gpue_dbuf* idx, uint64_t n,
                      gpue_dbuf* out, gpue_dbuf* out_nulls /* or NULL */);

/* ---- pinned double-buffered H2D ingest ----
 * north_star's "columnar batches pinned and streamed to HBM": two
 * hipHostMalloc staging buffers on the session's second stream; while chunk
 * k DMAs pinned->HBM, the host fills the other buffer — the morsel-driven
 * async-io shape of the reference's scan operator
 * (be/src/exec/pipeline/scan/scan_operator.h:40). */
typedef struct gpue_ingest gpue_ingest;
int gpue_ingest_create(gpue_session* s, uint64_t chunk_bytes, gpue_ingest** out);
/* page-locked host memory for producers that fill batches in place (zero
 * staging copy; DMA at full PCIe rate) */
int gpue_pinned_alloc(gpue_session* s, uint64_t bytes, void** host_ptr);
void gpue_pinned_free(void* host_ptr);
int gpue_ingest_push(gpue_ingest* g, const void* host, uint64_t bytes, gpue_dbuf* dst,
                     uint64_t dst_off);
int gpue_ingest_sync(gpue_ingest* g);
void gpue_ingest_destroy(gpue_ingest* g);

/* RLE page decode for int32 (storage ingress):
 * storage/rowset/rle_page.h header + base/bit/rle_encoding.h's
 * Parquet-style RLE/bit-pack hybrid at bit_width 32 (byte-aligned runs).
 * Two-phase device decode: run-table scan + binary-search parallel fill. */
int gpue_page_decode_rle_i32(gpue_session* s, gpue_dbuf* page, uint64_t n_values,
                             gpue_dbuf* out);
/* BOOL variant (bit_width 1, bit-packed literal groups; u8 output) */
int gpue_page_decode_rle_bool(gpue_session* s, gpue_dbuf* page, uint64_t n_values,
                              gpue_dbuf* out);
/* Frame-of-reference page decode (FOR_ENCODING,
 * frame_of_reference_coding.{h,cpp}): independent 128-value frames
 * (LE min + MSB-first bit-packed deltas; formats 0 min-delta / 1 ascending
 * prefix / 2 raw), decoded one block per frame with an LDS scan for the
 * ascending format. */
int gpue_page_decode_for_i32(gpue_session* s, gpue_dbuf* page, uint64_t n_values,
                             gpue_dbuf* out);
/* PlainPage numeric decode (plain_page.h:51,83-102,148-158): u32 LE count
 * + raw LE values; the fallback numeric encoding (encoding_info.cpp). */
int gpue_page_decode_plain_i32(gpue_session* s, gpue_dbuf* page, uint64_t n_values,
                               gpue_dbuf* out);
/* BinaryPlainPage -> BinaryColumn (binary_plain_page.h:28-46: string body +
 * u32 absolute-offset trailer + count). The dict page's dictionary format. */
int gpue_page_decode_binary_plain(gpue_session* s, gpue_dbuf* page, uint64_t n_values,
                                  gpue_dbuf* out_bytes, gpue_dbuf* out_offsets);
/* BinaryPrefixPage -> BinaryColumn (PREFIX_ENCODING,
 * binary_prefix_page.{h,cpp}: front coding, restart every 16 entries;
 * decode parallelizes per restart group). */
int gpue_page_decode_binary_prefix(gpue_session* s, gpue_dbuf* page, uint64_t n_values,
                                   gpue_dbuf* out_bytes, gpue_dbuf* out_offsets);

/* ---- ASOF join (reference LinearChainedAsofJoinHashMap,
 * join_hash_map_method.h:201-217 + AsofIndex, join_hash_table_descriptor.h:
 * 59-104 / .cpp:70-134). The selector routes every ASOF join here
 * (_get_fallback_method, join_hash_table.cpp:257-263). Equi-key lookup plus a
 * per-key temporal index sorted ascending (LT/LE) or descending (GT/GE),
 * probed with the reference's branchless lower-bound search; at most one
 * build match per probe row. GPU layout: open-addressing key slots + one
 * contiguous (asof_value, row) segment per key — binary search wants
 * contiguous sorted runs, not the CPU's pointer chains. Tie order among
 * duplicate (key, asof) pairs is unspecified in the reference (pdqsort is
 * unstable, comparator reads only asof_value); we pin the deterministic
 * refinement "smallest build row wins the boundary slot". */
#define GPUE_ASOF_LT 0 /* probe <  build: match smallest build value >  probe */
#define GPUE_ASOF_LE 1 /* probe <= build: match smallest build value >= probe */
#define GPUE_ASOF_GT 2 /* probe >  build: match largest  build value <  probe */
#define GPUE_ASOF_GE 3 /* probe >= build: match largest  build value <= probe */
typedef struct gpue_asof_table gpue_asof_table;
/* keys: (row_count+1) int32 equi keys, asof: (row_count+1) int64 temporal
 * values; row 0 is the sentinel "no match" row (never matched), as in the
 * reference's 1-based build rows. opcode: GPUE_ASOF_*. */
int gpue_asof_build_i32(gpue_session* s, gpue_dbuf* keys, gpue_dbuf* asof,
                        uint64_t row_count, int opcode, gpue_asof_table** out);
/* mode: GPUE_JOIN_INNER (matched rows only) or GPUE_JOIN_LEFT_OUTER (miss
 * emits build index 0), the reference's ASOF_INNER / ASOF_LEFT_OUTER
 * (join_hash_table.cpp:744). Two-call contract like gpue_join_probe_emit:
 * null outputs -> count only. Output ordered by probe row. */
int gpue_asof_probe_emit_i32(gpue_session* s, gpue_asof_table* t, gpue_dbuf* probe_keys,
                             gpue_dbuf* probe_asof, uint64_t n_rows, int mode,
                             gpue_dbuf* out_probe_idx, gpue_dbuf* out_build_idx,
                             uint64_t* match_count);
/* Nullable variants: is_nulls is a (row_count+1) u8 mask — the caller ORs the
 * equi-key and temporal null masks, and flagged build rows are skipped
 * exactly as the reference's is_null_row does
 * (join_hash_table_descriptor.h:447-456); null probe rows never match
 * (INNER drops them, LEFT_OUTER emits build row 0). */
int gpue_asof_build_nulls_i32(gpue_session* s, gpue_dbuf* keys, gpue_dbuf* asof,
                              gpue_dbuf* is_nulls, uint64_t row_count, int opcode,
                              gpue_asof_table** out);
int gpue_asof_probe_emit_nulls_i32(gpue_session* s, gpue_asof_table* t,
                                   gpue_dbuf* probe_keys, gpue_dbuf* probe_asof,
                                   gpue_dbuf* probe_nulls, uint64_t n_rows, int mode,
                                   gpue_dbuf* out_probe_idx, gpue_dbuf* out_build_idx,
                                   uint64_t* match_count);
int gpue_asof_table_destroy(gpue_asof_table* t);

/* ---- window functions: fn(...) OVER (PARTITION BY ... ORDER BY ... frame) --
 * The analytic operator (reference exec/analytor.cpp, exec/pipeline/analysis/):
 * one call evaluates 1..GPUE_WIN_MAX_FUNCS window functions that share one
 * PARTITION BY / ORDER BY clause. The entry does not sort: order_idx is a u32
 * permutation of [0, n_rows) listing the rows sorted by (partition keys, order
 * keys), exactly as gpue_topn writes it when called with the partition keys in
 * front of the order keys and limit >= n_rows; NULL = the rows are already in
 * that order. The buffer is trusted to be a permutation, but an index
 * >= n_rows is never dereferenced: the boundary pass latches the session's
 * device error word and the call returns GPUE_ERR_ARG with nothing else run.
 *
 * Keys: 0..GPUE_WIN_MAX_KEYS partition and 0..GPUE_WIN_MAX_KEYS order columns,
 * GPUE_PT_I32 / GPUE_PT_I64, with the nullable conventions of
 * gpue_group_agg_push (declared nullability + optional u8 null column). They
 * are used for equality only: sorted position i starts a partition iff i == 0
 * or some partition key differs from position i-1, and starts a peer group iff
 * it starts a partition or some order key differs. NULL equals NULL, the cell
 * under a NULL is never read, every 64-bit pattern is a legal key. No
 * partition keys: one partition. No order keys: all rows of a partition are
 * peers.
 *
 * Functions (all outputs int64; part_start/part_end/peer_start/peer_end are
 * sorted positions, inclusive; i is the row's sorted position):
 *   ROW_NUMBER  i - part_start + 1          RANK  peer_start - part_start + 1
 *   DENSE_RANK  peer groups in [part_start, i]
 *   NTILE       param0 = B >= 1; size = part_end - part_start + 1, q = size / B,
 *               r = size % B, rn0 = i - part_start: rn0/(q+1) + 1 if
 *               rn0 < r*(q+1), else r + (rn0 - r*(q+1))/q + 1
 *   COUNT_STAR, COUNT, SUM, MIN, MAX   aggregate over the frame [lo, hi]: COUNT
 *               counts non-NULL inputs, SUM wraps mod 2^64 (as GPUE_GA_SUM),
 *               SUM / MIN / MAX skip NULLs and are NULL when the frame holds
 *               no non-NULL input
 *   FIRST_VALUE, LAST_VALUE   the input at lo / at hi, a NULL passed through
 *   LAG, LEAD   param0 = k >= 0: the input at i - k / i + k if that position is
 *               inside the partition, else param1 if has_default, else NULL
 * Frames: GPUE_WF_ROWS: lo = max(part_start, i - frame_lo) (part_start when
 * GPUE_WIN_UNBOUNDED), hi = min(part_end, i + frame_hi) (part_end when
 * unbounded), frame_lo / frame_hi >= 0. GPUE_WF_RANGE: frame_lo must be
 * unbounded, frame_hi is 0 (hi = peer_end, SQL's default frame under ORDER BY)
 * or unbounded. MIN / MAX need frame_lo unbounded (no sliding minimum). The
 * frame fields are ignored for the ranking functions, NTILE and LAG / LEAD;
 * the input fields are ignored for functions that take no input.
 *
 * Output nullability is static: never for the ranking functions, NTILE,
 * COUNT_STAR, COUNT; iff the input was declared nullable for SUM, MIN, MAX,
 * FIRST_VALUE, LAST_VALUE; LAG / LEAD always, unless has_default is set and
 * the input is not nullable. A NULL output stores value 0, null byte 1,
 * otherwise null byte 0. A nullable output needs its null column; the null
 * column of a non-nullable output is ignored. The result for sorted position
 * i is written at out[order_idx[i]] (it lines up with the input columns), or
 * at out[i] with GPUE_WIN_OUT_SORTED.
 *
 * Scratch, allocated and freed inside the call, in bytes for n = n_rows:
 * n (boundary flags) + 8 n (part_start, peer_start) + 8 n more (part_end,
 * peer_end) unless every function is ROW_NUMBER / RANK / DENSE_RANK / LAG /
 * FIRST_VALUE, + per function: SUM 8 n, MIN / MAX 8 n, each + 4 n when its
 * input comes with a null column; COUNT 4 n when its input comes with a null
 * column; DENSE_RANK 4 n; the others 0; + 16 bytes per scan tile
 * (GPUE_WIN_TILE rows).
 *
 * GPUE_ERR_ARG, before any launch or allocation, for: n_part / n_order outside
 * 0..GPUE_WIN_MAX_KEYS, n_funcs outside 1..GPUE_WIN_MAX_FUNCS, an unknown
 * type, function, frame mode or flag, an illegal frame, NTILE with B < 1, a
 * negative k, n_rows >= 2^32, any buffer shorter than n_rows elements, a
 * missing input or output column, a missing null column for a nullable output,
 * a null buffer for a column declared non-nullable, an output that overlaps
 * another output or an input. n_rows == 0 returns GPUE_OK. Out of scope:
 * sliding MIN / MAX, RANGE with numeric offsets, IGNORE NULLS, CUME_DIST /
 * PERCENT_RANK, frames that exclude the current row. */
#define GPUE_WIN_MAX_FUNCS 8
#define GPUE_WIN_MAX_KEYS 4
#define GPUE_WIN_TILE 2048        /* rows per scan tile */
#define GPUE_WIN_MID 1024         /* tile aggregates per sweep of the middle pass */
#define GPUE_WFN_ROW_NUMBER 0
#define GPUE_WFN_RANK 1
#define GPUE_WFN_DENSE_RANK 2
#define GPUE_WFN_NTILE 3
#define GPUE_WFN_COUNT_STAR 4
#define GPUE_WFN_COUNT 5
#define GPUE_WFN_SUM 6
#define GPUE_WFN_MIN 7
#define GPUE_WFN_MAX 8
#define GPUE_WFN_FIRST_VALUE 9
#define GPUE_WFN_LAST_VALUE 10
#define GPUE_WFN_LAG 11
#define GPUE_WFN_LEAD 12
#define GPUE_WF_ROWS 0
#define GPUE_WF_RANGE 1
#define GPUE_WIN_UNBOUNDED (-1)   /* frame_lo / frame_hi */
#define GPUE_WIN_OUT_SORTED 1     /* flag: write the result of sorted position i at out[i] */
int gpue_window_eval(gpue_session* s, uint64_t n_rows, gpue_dbuf* order_idx /* u32 or NULL */,
                     gpue_dbuf** part_cols, gpue_dbuf** part_nulls, const int32_t* part_type,
                     const int32_t* part_nullable, int n_part,
                     gpue_dbuf** order_cols, gpue_dbuf** order_nulls, const int32_t* order_type,
                     const int32_t* order_nullable, int n_order,
                     const int32_t* fn /* GPUE_WFN_* */, gpue_dbuf** in_cols,
                     gpue_dbuf** in_nulls, const int32_t* in_type /* GPUE_PT_* */,
                     const int32_t* in_nullable, const int32_t* frame_mode,
                     const int64_t* frame_lo, const int64_t* frame_hi, const int64_t* param0,
                     const int64_t* param1, const int32_t* has_default, int n_funcs,
                     gpue_dbuf** out_cols /* int64 */, gpue_dbuf** out_nulls /* u8 */,
                     int flags);

/* ---- event timing on the session stream (bench roofline evidence) ---- */
int gpue_timer_start(gpue_session* s);
int gpue_timer_stop(gpue_session* s, float* ms_out);

#ifdef __cplusplus
}
#endif
#endif
