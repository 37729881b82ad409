/*
 * amdretrieval.h — C ABI of libamdretrieval.so (MI355X / gfx950 hybrid-retrieval kernels).
 *
 * The reference (Fan-Luo/Legal-RAG) is 100 % Python and has no FFI of its own
 * (SURVEY.md §8b); its native arithmetic lives in third-party wheels.  Each entry
 * point below therefore cites the reference CALL SITE whose native callee it
 * replaces.  Conventions: plain pointers and sizes only; every function returns
 * 0 on success or a negative AMDR_E* code, with a thread-local message available
 * from amdr_last_error(); the caller allocates all outputs; opaque handles are
 * safe for concurrent read-only searches (internally serialised per handle),
 * mutation (add/remove/replace/set_tokens/destroy) must not race with searches on the same handle.
 *
 * "_device" variants take DEVICE pointers and a hipStream_t passed as void*
 * (0 = the null stream); they enqueue work and return without synchronising,
 * and are graph-capturable once amdr_*_reserve() has sized the workspace
 * (reserve covers the "_device" workspace; the host-pointer calls size their own on first use).
 * A handle owns TWO workspaces: one for the "_device" calls, one for the plain
 * (host-pointer) calls.  "_device" calls on the same handle must be ordered with
 * respect to each other by the caller (same stream, or events between streams) —
 * the library only enqueues and cannot know when the caller's stream gets there.
 * Plain variants take HOST pointers, run on the handle's private stream inside
 * the handle's mutex and return after the results are in the host buffers: they
 * are safe to call from any number of threads, also while "_device" work of the
 * same handle is still in flight on another stream (different workspace).
 *
 * Batch size: every batched call serves any nq an int32 holds, memory permitting
 * (outputs and workspaces grow with nq; a failed allocation is AMDR_ENOMEM).  No
 * launch limit bounds it: a launch that carries the batch in the grid's y goes in
 * pieces of 65 535 queries on the same stream, so no grid dimension exceeds what
 * every HIP runtime accepts.
 */
#ifndef AMDRETRIEVAL_H
#define AMDRETRIEVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMDR_OK 0
#define AMDR_EINVAL (-1)   /* bad argument (null, shape, k out of range) */
#define AMDR_EHIP (-2)     /* a HIP runtime call failed; see amdr_last_error() */
#define AMDR_ENOMEM (-3)   /* device or host allocation failed */
#define AMDR_ENODEV (-4)   /* no usable gfx950 device */

#define AMDR_MAX_K 256      /* per-channel depth limit of the fused top-k kernels */
#define AMDR_MAX_DIM 1024   /* dense embedding dim limit (multiple of 4) */
#define AMDR_MAXSIM_DIM 128 /* ColBERT token dim (fixed by the kernel's register layout) */
#define AMDR_MAXSIM_QLEN 32 /* ColBERT query length after [MASK] padding */

typedef struct amdr_dense amdr_dense_t;
typedef struct amdr_dense_small amdr_dense_small_t;
typedef struct amdr_bm25 amdr_bm25_t;
typedef struct amdr_maxsim amdr_maxsim_t;
typedef struct amdr_tokenizer amdr_tokenizer_t;
typedef struct amdr_tokenizer_device amdr_tokenizer_device_t;
typedef struct amdr_graph amdr_graph_t;
typedef struct amdr_scope amdr_scope_t;
typedef struct amdr_vocab amdr_vocab_t;

/* ---- library ---------------------------------------------------------- */
const char* amdr_last_error(void);
int amdr_version(void);                     /* 10000*major + 100*minor + patch */
int amdr_device_count(int32_t* count);      /* number of visible HIP devices   */
int amdr_device_name(int32_t device, char* buf, int32_t buf_len); /* gcnArchName */
/* device workspace (re)allocations of every handle in the process since the library was loaded: a "_device" call
 * within a handle's reserve leaves it unchanged (tests read it around each call before they capture one) */
int amdr_workspace_growths(int64_t* out);

/* ---- dense channel: exact inner-product top-k -------------------------
 * Replaces faiss `index.add(emb)` (legalrag/retrieval/builders/faiss_builder.py:91,
 * incremental_dense_builder.py:62) and `index.search(q_vec, k)`
 * (legalrag/retrieval/dense_retriever.py:42, vector_store.py:169).
 * X: row-major fp32 [n, d] (rows L2-normalised by the encoder).  Results are
 * sorted by score descending, ties -> lower row id, padded with id -1 and
 * score -FLT_MAX when k > n (faiss convention). */
int amdr_dense_create(const float* X_host, int64_t n, int32_t d, int32_t device, amdr_dense_t** out);
/* adopt an existing device matrix without copying (the caller keeps ownership
 * and must keep it alive); used for shards generated in HBM.  The matrix is READ at creation (largest component and
 * row norm, for the fp16 first pass of large scans): the call synchronises the device first, so work that fills X on
 * any stream and was enqueued before the call is complete; the matrix must not change while the handle lives. */
int amdr_dense_create_from_device(const float* X_dev, int64_t n, int32_t d, int32_t device, amdr_dense_t** out);
int amdr_dense_add(amdr_dense_t* h, const float* X_host, int64_t n_add);
/* Remove n_remove rows (the reference has no removal: a corpus that shrinks takes `index.add` over everything again,
 * legalrag/retrieval/builders/faiss_builder.py:91, and then the reload of legalrag/retrieval/vector_store.py, which this
 * call replaces).  remove_ids[n_remove]: old row ids, strictly ascending, in [0, n); the surviving rows are renumbered
 * 0 .. n-n_remove-1 in their old order (ids close up: the faiss remove_ids convention of flat indexes, as
 * amdr_bm25_remove).  Removing every row is allowed and leaves the empty index (create accepts n = 0).
 * Afterwards the handle is what amdr_dense_create makes of the surviving rows: the same matrix bytes (amdr_dense_read_rows)
 * and the statistics of the fp16 first passes taken from zero over them — under add the largest component and row norm
 * only grow, here they can fall — hence the same ids and score bits from every entry point.  The short-corpus fp16 image
 * is dropped (made again on demand), the adaptation of the large scan's fp16 pass and its counters
 * (amdr_dense_hi_counters) start over, and a resident fp16 image (amdr_dense_image_build) is made again from the
 * compacted matrix — its 32-row tiles hold other rows now — or dropped when the index is empty or its statistics are no
 * longer finite.  The work is one ordered compaction of the matrix at HBM speed into a NEW buffer (csrc/rows_compact.hip:
 * every surviving byte read once and written once; no atomics, deterministic) and the statistics pass; host work is
 * proportional to n_remove.  Capacity afterwards equals the survivors; a later add grows as it does today.
 * AMDR_EINVAL: null handle, a handle from amdr_dense_create_from_device, n_remove < 0, null remove_ids, an id outside
 * [0, n), ids not strictly ascending.  n_remove == 0 is a no-op that reads nothing.  A failed remove (AMDR_EINVAL,
 * AMDR_ENOMEM, AMDR_EHIP) leaves the handle as it was and searchable.  The price of that: the old and the new matrix
 * (and 8 B per removed id) are resident for the length of the call, so it can return AMDR_ENOMEM on a device where the
 * matrix itself fits.  Runs inside the handle's mutex.  It is a mutation in the sense of the rule at the top of this
 * file: "_device" work of the handle still in flight is the caller's to finish first (the matrix it reads is freed),
 * captured graphs hold the old buffer and sizes and must be reserved and captured again, workspaces are never shrunk.
 * Row ids held by others — the graph tables node_row / row_node / row_norm of amdr_graph_create, scope tables, row2uid
 * maps of the fusion calls — name the old rows and are the caller's to rebuild. */
int amdr_dense_remove(amdr_dense_t* h, const int64_t* remove_ids, int64_t n_remove);
/* Device time of the compaction kernel of the last successful amdr_dense_remove, in ms between two events on the
 * handle's stream (scripts/bench_store_remove.py sets it against the kernel's algorithmic bytes); -1 before the first
 * remove. */
int amdr_dense_remove_kernel_ms(amdr_dense_t* h, double* ms);
/* Replace n_rep rows under their ids: an amended article keeps its row (the reference has no update: its builders skip a
 * chunk id they have seen, legalrag/retrieval/builders/incremental_dense_builder.py:50-51, so an amendment takes a
 * rebuild).
 * replace_ids[n_rep]: old row ids, strictly ascending, in [0, n); row replace_ids[i] takes X_host[i, :].  No id moves, so
 * row ids held by others (graph tables, scope tables, row2uid maps) still name the same chunks — only what is derived
 * from a row's VALUES (the graph's row_norm) is the caller's to refresh.
 * Afterwards the handle is what amdr_dense_create makes of the edited matrix: the same matrix bytes
 * (amdr_dense_read_rows) and the statistics of the fp16 first passes taken again from zero over all rows — the largest
 * component and row norm can fall, as under remove — hence the same ids and score bits from every entry point.  The
 * short-corpus fp16 image is dropped (made again on demand), the adaptation of the large scan's fp16 pass and its
 * counters start over as in amdr_dense_remove, and a resident fp16 image stays current: converted again from the first
 * touched 32-row tile on, all of it when the power-of-two scale changed, dropped when the statistics are no longer
 * finite.  The work: the new rows and ids are staged on the device, then one scatter kernel in 16-byte units writes the
 * matrix IN PLACE (csrc/rows_compact.hip: every replaced byte read once and written once, nothing else moves; no atomics,
 * deterministic), then the statistics pass over the matrix.
 * AMDR_EINVAL: null handle, a handle from amdr_dense_create_from_device, n_rep < 0, null replace_ids or X_host,
 * n_rep > n, an id outside [0, n), ids not strictly ascending.  n_rep == 0 is a no-op that reads nothing.  Everything that
 * can fail happens before the scatter is enqueued, so a failed replace (AMDR_EINVAL, AMDR_ENOMEM, AMDR_EHIP) leaves the
 * handle as it was and searchable.  Transient memory: the staged rows and ids (4 d + 8 bytes per replaced row) for the
 * length of the call; no second matrix.  Runs inside the handle's mutex.  It is a mutation in the sense of the rule at
 * the top of this file: "_device" work of the handle still in flight is the caller's to finish first (it would read a
 * half-written matrix), and captured graphs must be reserved and captured again (the statistics they were routed by
 * changed).  The row count does not change, so no workspace grows. */
int amdr_dense_replace(amdr_dense_t* h, const int64_t* replace_ids, const float* X_host, int64_t n_rep);
/* Device time of the scatter kernel of the last successful amdr_dense_replace, in ms between two events on the handle's
 * stream (scripts/bench_replace.py); -1 before the first replace. */
int amdr_dense_replace_kernel_ms(amdr_dense_t* h, double* ms);
int amdr_dense_ntotal(const amdr_dense_t* h, int64_t* n);
int amdr_dense_dim(const amdr_dense_t* h, int32_t* d);
int amdr_dense_reserve(amdr_dense_t* h, int32_t nq_max, int32_t k_max);
int amdr_dense_search(amdr_dense_t* h, const float* Q_host, int32_t nq, int32_t k,
                      float* scores_host, int64_t* ids_host);
int amdr_dense_search_device(amdr_dense_t* h, const float* Q_dev, int32_t nq, int32_t k,
                             float* scores_dev, int64_t* ids_dev, void* stream);
/* scores of an explicit candidate list: out[q, j] = <Q[q], X[rows[q, j]]>, -FLT_MAX for
 * rows outside [0, n).  Building block for GraphRetriever's candidate rescoring
 * (legalrag/retrieval/graph_retriever.py:177-191 re-embeds up to graph_limit=800 candidate
 * texts per query and takes cosines; the embeddings are already resident here). */
int amdr_dense_score_rows(amdr_dense_t* h, const float* Q_host, int32_t nq, const int64_t* rows_host, int32_t m,
                          float* scores_host);
/* copy rows [row0, row0+nrows) back to the host (used by parity tests to run
 * the oracle on exactly the matrix that is resident in HBM) */
int amdr_dense_read_rows(const amdr_dense_t* h, int64_t row0, int64_t nrows, float* out_host);
/* Which kernels a search of nq queries at depth k would launch on this index, and how the work
 * is cut (e.g. "dense_panel_scores_kernel nb=6 parts=7 blocks=2044 + scores_pair_topk_kernel";
 * the top-k kernel named is the one the launch picks):
 * written NUL-terminated into buf.  No device work.  bench.py names its roofline kernel with it. */
int amdr_dense_plan_info(const amdr_dense_t* h, int32_t nq, int32_t k, char* buf, int32_t buf_len);
/* Host-only (no device is touched): on an [n, d] matrix, out6[0..2] = the bytes amdr_dense_reserve(nq_max, k_max) sizes
 * for the "_device" calls — score / tile-maxima matrix, slab lists, candidate-tile lists — and out6[3..5] = the most any
 * pass (full chunks and the remainder) of amdr_dense_search_device(nq, k) uses, whichever form the call takes.  A test
 * holds out6[3+i] <= out6[i] for every nq <= nq_max, k <= k_max (tests/test_abi.py). */
int amdr_dense_workspace_plan(int64_t n, int32_t d, int32_t nq_max, int32_t k_max, int32_t nq, int32_t k, int64_t* out6);
/* Large scans (chunk matrix far beyond the caches, >= 5 queries): the first pass of the two-level top-k runs on the
 * fp16 matrix instructions over fp16 roundings of both operands, 64 queries per scan; its candidate cut is widened by a
 * proven rounding bound and the second pass is the exact fp32 kernel, so ids and score bits are those of the exact
 * forms (csrc/dense_hi.hip).  A query whose cut the bound does not separate sends its batch through the exact first
 * pass as well (decided on the device).  The width of the candidate cut adapts per handle: k + max(k, 22 / 54 / 96)
 * + 1 tiles per query (levels 0-2).  One unresolved query sends its whole pass (<= 64 queries) through the exact chain,
 * so passes are what is counted: more than 10 % of >= 4 passes flagged moves the handle up a level, at the top level
 * more than half make it give the fp16 pass up (exact passes from then on); AMDR_DENSE_HI_LEVEL pins the level.
 * out6[0] = queries that took the fp16 first pass since creation, out6[1] = those it could not resolve, out6[2] =
 * current level, out6[3] = 1 while the pass is in use, out6[4] = passes, out6[5] = passes whose flag went up.
 * Synchronises the device.  The matrix wrapped by amdr_dense_create_from_device must not change while the handle
 * lives (its largest component and row norm are measured at creation). */
int amdr_dense_hi_counters(amdr_dense_t* h, int64_t* out6);
/* Optional resident fp16 image of the matrix for the fp16 first pass of large scans (`index.search`,
 * legalrag/retrieval/dense_retriever.py:42): for every 32-row tile and 64-component chunk the halves fp16(x * 2^-e) that the
 * pass otherwise rounds from the fp32 matrix in registers, in the order its kernel reads them — the pass then streams half
 * the bytes and computes the same tile maxima bit for bit, so every id and score bit of a search is what it is without the
 * image (the exact re-scoring still reads the fp32 matrix, which stays).  Memory: ceil(n / 32) * 32 * d * 2 bytes, owned
 * by the handle, not workspace (amdr_dense_workspace_plan / amdr_workspace_growths do not count it).
 * build: synchronous (allocates, converts, waits); a no-op on a handle whose image is current; AMDR_EINVAL for a width
 * the fp16 first pass does not support (d % 128 != 0 or d < 128), an empty index, or a matrix whose statistics are not
 * finite (an infinite component or row norm, or a largest component outside 2^+-99); allowed on handles from
 * amdr_dense_create_from_device.  No search ever builds or allocates it.  amdr_dense_add keeps a present image current: it
 * converts the new rows, or the whole matrix when the add changes the matrix's power-of-two scale or the image has no
 * room; if the add leaves the statistics non-finite the image is dropped.  AMDR_DENSE_HI_IMAGE=0 makes searches ignore it.
 * drop: frees it (waits for the device).  info: out4[0] = 1 if present, out4[1] = bytes allocated, out4[2] = rows covered,
 * out4[3] = e of the scale 2^-e it was converted with. */
int amdr_dense_image_build(amdr_dense_t* h);
int amdr_dense_image_drop(amdr_dense_t* h);
int amdr_dense_image_info(amdr_dense_t* h, int64_t* out4);
/* HIP-event bracket around the scan kernel alone (not the merge), recorded on
 * the stream each search is launched on; used by bench.py for the roofline.
 * begin() arms up to max_launches event pairs, end() returns the summed scan
 * time and the number of launches measured since begin(). */
int amdr_dense_profile_begin(amdr_dense_t* h, int32_t max_launches);
int amdr_dense_profile_end(amdr_dense_t* h, double* total_ms, int32_t* launches);
int amdr_dense_destroy(amdr_dense_t* h);

/* ---- BM25 channel: Okapi scoring over term-major CSR postings ----------
 * Replaces `BM25Okapi.get_scores(tokens)` + the full Python sort
 * (legalrag/retrieval/bm25_retriever.py:74-75).  float64 throughout, no FMA
 * contraction; per document the query tokens are accumulated in query order
 * with duplicates counted, so scores are bit-identical to rank_bm25's numpy
 * expression.  Ties -> lower doc id; zero-score docs ARE returned.
 * term_ptr[n_terms+1] indexes post_doc/post_tf (ascending doc id per term);
 * idf already has rank_bm25's epsilon floor applied; every idf must be finite (AMDR_EINVAL otherwise).
 * Resident per posting: doc id (4 B) + fp64 factor (8 B), which the searches read, + tf (4 B); per document: its length
 * (4 B).  tf and the lengths are kept only for amdr_bm25_add / amdr_bm25_remove / amdr_bm25_replace, which recompute every factor from them: 16 B per posting
 * of HBM instead of 12, + 4 B per document. */
int amdr_bm25_create(const int64_t* term_ptr, const int32_t* post_doc, const int32_t* post_tf,
                     const double* idf, const int32_t* doc_len, int64_t n_terms, int64_t n_docs,
                     double avgdl, double k1, double b, int32_t device, amdr_bm25_t** out);
int amdr_bm25_ndocs(const amdr_bm25_t* h, int64_t* n);
/* Append n_add documents (replaces the full re-fit + reload of an ingest, legalrag/retrieval/builders/
 * incremental_bm25_builder.py:70-79 followed by bm25_retriever.py:44-56).  n_terms >= the handle's: old term ids keep
 * their meaning, new terms take the ids behind them.  term_ptr_add[n_terms+1] / post_doc_add / post_tf_add: the added
 * documents' own term-major CSR over the NEW term table, post_doc_add holding local ids 0 .. n_add-1, strictly ascending
 * per term; doc_len_add[n_add]; idf[n_terms]: the whole new vector, floor applied, computed by the caller as for create
 * (native code takes no logarithm); avgdl: the caller's new value.  New document ids are n_docs .. n_docs+n_add-1.
 * Afterwards the handle is what amdr_bm25_create makes of the concatenated index: term_ptr, post_doc, post_w and idf are
 * the same bytes, hence the same ids and score bits from every entry point.  N and avgdl are corpus-global, so every
 * factor changes: the call is one device pass over ALL resident postings (each term's list grows at its tail, each factor
 * is recomputed with the new avgdl) plus host work proportional to the add — it validates the add's arrays only.
 * AMDR_EINVAL: null handle, n_add < 0, null arrays with n_add > 0, n_terms below the handle's, term_ptr_add[0] != 0 or
 * not monotone, a post_doc_add outside [0, n_add) or not strictly ascending within a term, a non-finite idf, a
 * non-finite or non-positive avgdl, n_docs + n_add >= 2^31; n_add == 0 is a no-op that reads nothing.  A failed add
 * (AMDR_EINVAL, AMDR_ENOMEM, AMDR_EHIP) leaves the handle as it was and searchable.  The price of that: the new arrays
 * are built beside the old ones and swapped in after the handle's stream has finished, so for the length of the call
 * the device holds a second copy of the index (16 B per posting, 4 B per document, 16 B per term) and the call can
 * return AMDR_ENOMEM where the index itself fits.  Runs inside the handle's mutex: host-pointer searches from other
 * threads serialise against it.  It is a mutation in the sense of the rule at the top of this file: "_device" work of
 * the handle still in flight is the caller's to finish first (the arrays it reads are freed); workspaces are sized per
 * call from n_docs, so an eager "_device" call after an add grows its workspace if it has to (amdr_workspace_growths
 * shows it), and a captured graph holds the old arrays and sizes and must be re-reserved (amdr_bm25_reserve) and
 * captured again.  The arrival counters of the one-launch serving step stay as they are.  A successful add drops the
 * token stream (amdr_bm25_set_tokens); amdr_bm25_add_carry below keeps it current instead. */
int amdr_bm25_add(amdr_bm25_t* h, const int64_t* term_ptr_add, const int32_t* post_doc_add, const int32_t* post_tf_add,
                  const double* idf, const int32_t* doc_len_add, int64_t n_terms, int64_t n_add, double avgdl);
/* Remove n_remove documents (the reference has no removal: a corpus that shrinks takes the full re-fit + reload of
 * legalrag/retrieval/builders/incremental_bm25_builder.py:70-79 followed by bm25_retriever.py:44-56, which this call
 * replaces).  remove_ids[n_remove]: old document ids, strictly ascending, in [0, n_docs); n_remove < n_docs (an index
 * keeps a document, as create demands).  The surviving documents are renumbered 0 .. n_docs-n_remove-1 in their old order
 * (ids close up: the faiss remove_ids convention of flat indexes).  term_map[n_terms]: the new id of each old term or -1,
 * the ids >= 0 a bijection onto [0, n_terms_new) — a re-fit of the survivors drops the terms whose documents are all gone
 * and may order the rest differently; null is the identity: n_terms_new == n_terms and an emptied term keeps its id with
 * an empty list.  idf[n_terms_new]: the whole new vector, floor applied, computed by the caller as for create (native
 * code takes no logarithm); avgdl: the caller's new value.
 * Afterwards the handle is what amdr_bm25_create makes of the surviving documents' index with the terms renumbered by
 * the map, each list ascending: term_ptr, post_doc, post_tf, post_w, idf and doc_len are the same bytes (amdr_bm25_read),
 * hence the same ids and score bits from every entry point.  N, avgdl and every idf are corpus-global, so every factor
 * changes: the call is two device passes over ALL resident postings (count, then scatter with the factor recomputed; the
 * tiles of 2 048 old postings and the short scans between them are described in csrc/bm25_update.hip) plus host work
 * proportional to n_terms + n_remove — it validates the call's arrays only.  No atomics: the result is deterministic.
 * AMDR_EINVAL: null handle, n_remove < 0, null remove_ids or (n_terms_new > 0) null idf, n_remove >= n_docs, an id outside
 * [0, n_docs), ids not strictly ascending, n_terms_new outside [0, n_terms], a null map with n_terms_new != n_terms, a map
 * value below -1 or >= n_terms_new, two terms on one new id, a new id no term maps to, a non-finite idf, a non-finite or
 * non-positive avgdl — and a term mapped to -1 that still has a surviving posting, which only the device sees: the
 * counting passes raise a flag that is read before the swap.  n_remove == 0 is a no-op that reads nothing.  A failed
 * remove (AMDR_EINVAL, AMDR_ENOMEM, AMDR_EHIP) leaves the handle as it was and searchable; the price is the add's: the
 * new arrays are built beside the old ones and swapped in after the handle's stream has finished (for the length of the
 * call the device also holds 2 B per old posting, 4 B per old document and 8 B per term of scratch).  Runs inside the
 * handle's mutex.  It is a mutation in the sense of the rule at the top of this file, and the rules for in-flight
 * "_device" work, for workspaces and for captured graphs are those of amdr_bm25_add: finish the work first, reserve and
 * capture again.  The arrival counters of the one-launch serving step stay as they are.  A successful remove drops the
 * token stream (amdr_bm25_set_tokens); amdr_bm25_remove_carry below keeps it current instead. */
int amdr_bm25_remove(amdr_bm25_t* h, const int64_t* remove_ids, int64_t n_remove, const int32_t* term_map,
                     int64_t n_terms_new, const double* idf, double avgdl);
/* Summed device time of the passes of the last successful amdr_bm25_remove, in ms between events on the handle's stream
 * (scripts/bench_bm25_remove.py sets it against the passes' algorithmic bytes); -1 before the first remove. */
int amdr_bm25_remove_kernel_ms(amdr_bm25_t* h, double* ms);
/* Replace n_rep documents under their ids: an amended article keeps its id (the reference has no update: its builder
 * skips a chunk id it has seen, legalrag/retrieval/builders/incremental_bm25_builder.py:56-57, so an amendment takes the
 * full re-fit + reload).  replace_ids[n_rep]: old document ids, strictly ascending, in [0, n_docs); n_rep <= n_docs.  The new
 * documents come as their own term-major CSR over the NEW term table, as in amdr_bm25_add: term_ptr_add[n_terms_new + 1] /
 * post_doc_add / post_tf_add, post_doc_add holding local ids 0 .. n_rep-1, strictly ascending per term, local i being
 * document replace_ids[i]; doc_len_add[n_rep].  term_map[n_terms]: the new id of each old term or -1, injective, as in
 * amdr_bm25_remove — a re-fit of the edited corpus drops the terms whose last document lost them and may order the rest
 * differently; null is the identity on the old terms with the new terms behind them (n_terms_new >= n_terms; an emptied
 * term keeps its id with an empty list).  New ids that no old term maps to are NEW terms: their lists come from the add
 * alone.  idf[n_terms_new] and avgdl are the caller's values, as in both other updates (native code takes no logarithm).
 * Afterwards every new term's list is the merge by document id of its old term's surviving postings (the documents not
 * in replace_ids) and the add's postings at replace_ids[local]; doc_len[replace_ids[i]] = doc_len_add[i]; every factor
 * is recomputed.  The handle is what amdr_bm25_create makes of the edited index: term_ptr, post_doc, post_tf, post_w, idf
 * and doc_len are the same bytes (amdr_bm25_read), hence the same ids and score bits from every entry point.  No
 * document id moves, so tables that name documents stay valid.
 * The work: one count and one scatter over ALL resident postings (the remove's tiles of 2 048 old postings and its
 * counting pass) plus one pass over the add's postings — one pass fewer than a remove followed by an add — and host work
 * proportional to n_terms + n_rep + the add's postings: it validates the call's arrays only.  A posting's place is a sum
 * of counts and one binary search in the other source's list (csrc/bm25_replace_rule.hpp): no atomics, deterministic.
 * AMDR_EINVAL: null handle, n_rep < 0, a null array the sizes say is read, n_rep > n_docs, an id outside [0, n_docs), ids
 * not strictly ascending, n_terms_new outside [0, 2^31), a null map with n_terms_new < n_terms, a map value below -1 or
 * >= n_terms_new, two terms on one new id, term_ptr_add[0] != 0 or not monotone, a post_doc_add outside [0, n_rep) or
 * not strictly ascending within a term, a non-finite idf, a non-finite or non-positive avgdl — and a term mapped to -1
 * that still has a surviving posting, which only the device sees: the counting passes raise a flag that is read before
 * the swap.  n_rep == 0 is a no-op that reads nothing.  A failed replace (AMDR_EINVAL, AMDR_ENOMEM, AMDR_EHIP) leaves the
 * handle as it was and searchable.  Transient memory: the new arrays are built beside the old ones and swapped in after
 * the handle's stream has finished (a second copy of the index: 16 B per posting, 4 B per document, 16 B per term), plus
 * the scratch of the remove (2 B per old posting, 4 B per document, 8 B per old term), the add's CSR (8 B per added
 * posting, 8 B per new term), 12 B per new term and 12 B per replaced document.  Runs inside the handle's mutex.  It is
 * a mutation in the sense of the rule at the top of this file, and the rules for in-flight "_device" work and for
 * captured graphs are those of amdr_bm25_add: finish the work first, reserve and capture again.  n_docs does not change,
 * so no workspace grows.  The arrival counters of the one-launch serving step stay as they are.  A successful replace
 * drops the token stream (amdr_bm25_set_tokens); amdr_bm25_replace_carry below keeps it current instead. */
int amdr_bm25_replace(amdr_bm25_t* h, const int64_t* replace_ids, int64_t n_rep, const int64_t* term_ptr_add,
                      const int32_t* post_doc_add, const int32_t* post_tf_add, const int32_t* doc_len_add,
                      const int32_t* term_map, int64_t n_terms_new, const double* idf, double avgdl);
/* Summed device time of the passes of the last successful amdr_bm25_replace, in ms between events on the handle's stream
 * (scripts/bench_replace.py sets it against the passes' algorithmic bytes); -1 before the first replace. */
int amdr_bm25_replace_kernel_ms(amdr_bm25_t* h, double* ms);
/* The carrying forms of the three updates: the plain call's arguments in the plain call's order, then the token arguments.
 * The index part IS the plain call's (one body, csrc/bm25_update.hip): the same validation, the same bytes afterwards, the
 * same counters and the same *_kernel_ms.  What differs is the token stream of amdr_bm25_set_tokens:
 *   with a resident stream, a successful call leaves the stream that amdr_bm25_set_tokens makes of the edited corpus, byte
 *   for byte (amdr_bm25_read_tokens), instead of dropping it, and amdr_bm25_tokens_info reports (1, the new token count);
 *   without a resident stream the call is the plain call: the token arrays are validated and otherwise unused, and no
 *   stream appears.
 * tok_ptr_add[n_add + 1] (n_rep + 1 in a replace), tok_add[tok_ptr_add[last]]: local document i's text as term ids over the
 * NEW term table, in text order; tok_add may be null when the arrays hold no token.  A removal brings no text and takes no
 * new array.  The new stream:
 *   add      the old stream with the added documents behind it (old term ids keep their meaning);
 *   remove   the survivors' documents in their old order, every token t rewritten to term_map[t] (null: the identity);
 *   replace  document replace_ids[i] takes local i's tokens, every other document keeps its own, rewritten through
 *            term_map (null: the identity);
 * and in all three the new doc_ptr is the exclusive 64-bit scan of the NEW doc_len.  Every position is 64-bit: a stream may
 * pass 2^31 tokens.  The work is one device pass over the NEW tokens (tiles of 2 048 output tokens, csrc/tok_carry_rule.hpp:
 * one 4 B read, one 4 B gather of the term map, one 4 B write per token; no atomics, deterministic) plus host work
 * proportional to the update: the add's token arrays are validated as amdr_bm25_set_tokens validates a stream, against
 * doc_len_add and n_terms (n_terms_new) — AMDR_EINVAL, handle unchanged: a null tok_ptr_add, a null tok_add with tokens,
 * tok_ptr_add[0] != 0 or not monotone, a run that is not doc_len_add[i] tokens long, a token outside the new term table.
 * What only the device sees — a token of a surviving document whose term is mapped to -1 (the flag the counting passes
 * raise for such a posting), a gather index outside its array — is read before the swap: AMDR_EINVAL, index and stream as
 * they were.  Staging: the new stream is built beside the old one and committed together with the index, after the
 * handle's stream has finished, and nothing can fail after that; any failure, AMDR_ENOMEM for the second copy of the
 * stream included, fails the whole update and leaves index AND stream as they were.  Transient memory on top of the plain
 * call's: the second copy of the stream (4 B per new token and 8 B per document), the add's stream (4 B per added token,
 * 8 B per added document), 8 B per document of scratch for the scan, and in a remove 4 B per surviving document.
 * n_add / n_remove / n_rep == 0 is the plain call's no-op: nothing is read and the stream stays.  Mutations in the sense of
 * the rule at the top of this file, as the plain calls are. */
int amdr_bm25_add_carry(amdr_bm25_t* h, const int64_t* term_ptr_add, const int32_t* post_doc_add, const int32_t* post_tf_add,
                        const double* idf, const int32_t* doc_len_add, int64_t n_terms, int64_t n_add, double avgdl,
                        const int64_t* tok_ptr_add, const int32_t* tok_add);
int amdr_bm25_remove_carry(amdr_bm25_t* h, const int64_t* remove_ids, int64_t n_remove, const int32_t* term_map,
                           int64_t n_terms_new, const double* idf, double avgdl);
int amdr_bm25_replace_carry(amdr_bm25_t* h, const int64_t* replace_ids, int64_t n_rep, const int64_t* term_ptr_add,
                            const int32_t* post_doc_add, const int32_t* post_tf_add, const int32_t* doc_len_add,
                            const int32_t* term_map, int64_t n_terms_new, const double* idf, double avgdl,
                            const int64_t* tok_ptr_add, const int32_t* tok_add);
/* Summed device time of the carry passes (the scan of the new lengths and the pass over the new tokens) of the last
 * successful carrying update that carried a stream, in ms between events on the handle's stream
 * (scripts/bench_tokens_carry.py sets it against the pass's algorithmic bytes); -1 before the first one. */
int amdr_bm25_carry_kernel_ms(amdr_bm25_t* h, double* ms);
/* Replaces so far (amdr_bm25_info keeps its six words: a replace touches neither [3] nor [5]). */
int amdr_bm25_replaces(amdr_bm25_t* h, int64_t* n);
/* out6: [0] n_docs, [1] n_terms, [2] nnz (postings), [3] adds so far, [4] the tile length in postings of the merge
 *       kernel and of the remove's passes, [5] removes so far (an add does not touch [5], a remove does not touch [3]) */
int amdr_bm25_info(amdr_bm25_t* h, int64_t* out6);
/* Device time of the merge kernel of the last successful amdr_bm25_add, in ms between two events on the handle's stream
 * (scripts/bench_bm25_add.py sets it against the kernel's algorithmic bytes); -1 before the first add. */
int amdr_bm25_add_kernel_ms(amdr_bm25_t* h, double* ms);
/* Copies the resident arrays to the host: term_ptr[n_terms+1], post_doc / post_tf / post_w[nnz], idf[n_terms],
 * doc_len[n_docs] (sizes from amdr_bm25_info); any pointer may be null.  The only way to see what a handle holds. */
int amdr_bm25_read(amdr_bm25_t* h, int64_t* term_ptr, int32_t* post_doc, int32_t* post_tf, double* post_w, double* idf,
                   int32_t* doc_len);
/* The token stream (forward index) of the corpus, for phrase constraints (amdr_phrase_lists below; the reference keeps no
 * token order anywhere).  doc_ptr[n_docs + 1], tokens[doc_ptr[n_docs]]: document d's text, as the index tokeniser cut it,
 * is the term ids tokens[doc_ptr[d] .. doc_ptr[d + 1]).  4 B per token and 8 B per document on the device.  Validated on
 * the host, AMDR_EINVAL, handle unchanged: a null handle or array, doc_ptr[0] != 0 or doc_ptr not monotone, a token outside
 * [0, n_terms), doc_ptr[d + 1] - doc_ptr[d] != doc_len[d] for any d (the handle's doc_len is read once for this: the check
 * that catches a stream made for another state of the index).  A second call replaces the stream.  amdr_bm25_add /
 * _remove / _replace renumber documents and terms: a SUCCESSFUL call of any of them DROPS the stream (a failed one leaves
 * it) and the caller sets a new one, or calls their carrying forms (amdr_bm25_*_carry), which keep it current.  Setting a stream is a mutation in the sense of the rule at the top of this file.
 * Searches and amdr_term_scope* calls without virtual lists behave exactly as without a stream. */
int amdr_bm25_set_tokens(amdr_bm25_t* h, const int64_t* doc_ptr, const int32_t* tokens);
/* out2: [0] 1 if a token stream is resident else 0, [1] its token count (0 without one) */
int amdr_bm25_tokens_info(amdr_bm25_t* h, int64_t* out2);
/* Copies the resident stream to the host: doc_ptr[n_docs + 1], tokens[out2[1]]; either pointer may be null.
 * AMDR_EINVAL when no stream is resident. */
int amdr_bm25_read_tokens(amdr_bm25_t* h, int64_t* doc_ptr, int32_t* tokens);
int amdr_bm25_reserve(amdr_bm25_t* h, int32_t nq_max, int32_t k_max, int64_t total_terms_max);
/* Host-only (no device is touched): on a corpus of n_docs documents, out2[0] = the slab-list bytes amdr_bm25_reserve
 * (nq_max, k_max) sizes for the "_device" calls, out2[1] = the bytes amdr_bm25_search_device(nq, k) uses.  A test holds
 * out2[1] <= out2[0] for every nq <= nq_max, k <= k_max (tests/test_abi.py). */
int amdr_bm25_workspace_plan(int64_t n_docs, int32_t nq_max, int32_t k_max, int32_t nq, int32_t k, int64_t* out2);
/* which kernels a search of nq queries at depth k would launch and how the corpus is cut into slabs (NUL-terminated;
 * no device work) */
int amdr_bm25_plan_info(const amdr_bm25_t* h, int32_t nq, int32_t k, char* buf, int32_t buf_len);
/* queries as CSR: q_terms[q_ptr[i] .. q_ptr[i+1]) = term ids of query i in
 * token order (unknown tokens: any negative id, they score 0) */
int amdr_bm25_search(amdr_bm25_t* h, const int32_t* q_terms, const int64_t* q_ptr, int32_t nq, int32_t k,
                     double* scores_host, int64_t* ids_host);
int amdr_bm25_search_device(amdr_bm25_t* h, const int32_t* q_terms_dev, const int64_t* q_ptr_dev,
                            int32_t nq, int32_t k, double* scores_dev, int64_t* ids_dev, void* stream);
/* dense score vectors [nq, n_docs] == BM25Okapi.get_scores per query */
int amdr_bm25_scores(amdr_bm25_t* h, const int32_t* q_terms, const int64_t* q_ptr, int32_t nq,
                     double* scores_host);
int amdr_bm25_destroy(amdr_bm25_t* h);

/* ---- BM25 query tokeniser + vocabulary lookup, batched (host code) -------
 * Replaces, per query, `tokens = list(jieba.cut(query))` and the per-token vocabulary lookup of
 * `BM25Okapi.get_scores` (legalrag/retrieval/bm25_retriever.py:73-74) for text WITHOUT Han characters — the
 * case jieba's default mode decides without its dictionary (rule: legal-rag_amd/text.py, which stays the executable
 * specification; csrc/tokenize.cpp).  Queries are not lower-cased (the reference does not).  A query holding a Han
 * character is not tokenised: needs_segmenter[q] = 1, it gets no terms, and the caller takes its own segmenter.
 * vocab: n_terms UTF-8 strings, term i = vocab_blob[vocab_offsets[i] .. vocab_offsets[i+1]).
 * encode: queries as one UTF-8 blob + offsets [nq+1]; writes the CSR amdr_bm25_search takes — term_ids (capacity:
 * the blob's byte length always suffices; unknown token = -1) and q_ptr [nq+1].  No device work; thread-safe. */
int amdr_tokenizer_create(const char* vocab_blob, const int64_t* vocab_offsets, int64_t n_terms, amdr_tokenizer_t** out);
int amdr_tokenizer_encode(const amdr_tokenizer_t* t, const char* text_blob, const int64_t* text_offsets, int32_t nq,
                          int32_t* term_ids, int64_t capacity, int64_t* q_ptr, int32_t* needs_segmenter);
/* the same for queries joined by ONE NUL byte each (nq - 1 separators in n_bytes; a caller with a list of Python strings
 * builds this blob with two C-level operations — "\0".join(qs).encode() — instead of one encode per query).  Both forms
 * cut a batch into ranges of queries for a small persistent pool of worker threads (AMDR_TOKENIZER_THREADS, default: the
 * hardware's, at most 32; one worker per 256 queries) and splice the ranges' terms by a prefix sum. */
int amdr_tokenizer_encode_joined(const amdr_tokenizer_t* t, const char* text_blob, int64_t n_bytes, int32_t nq,
                                 int32_t* term_ids, int64_t capacity, int64_t* q_ptr, int32_t* needs_segmenter);
/* the same for queries that lie where they are: texts[q] = the n_bytes[q] UTF-8 bytes of query q (no blob is built; a
 * Python caller takes the pointers from the str objects themselves, csrc/pystrings.c) */
int amdr_tokenizer_encode_ptrs(const amdr_tokenizer_t* t, const char* const* texts, const int64_t* n_bytes, int32_t nq,
                               int32_t* term_ids, int64_t capacity, int64_t* q_ptr, int32_t* needs_segmenter);
/* byte spans of one text's tokens (tests compare them with text.jieba_cut); *n_tokens = -1: Han text */
int amdr_tokenizer_spans(const char* text, int64_t n_bytes, int32_t* starts, int32_t* ends, int32_t capacity,
                         int32_t* n_tokens);
/* Han text on the same handle.  Replaces the same call site for queries that hold a Han character
 * (legalrag/retrieval/bm25_retriever.py:73-74; the index side of the same tokens is bm25_builder.py:43) by one of the
 * two declared stand-ins of legal-rag_amd/text.py, which stays the executable specification:
 *   AMDR_HAN_FLAG  the default: such a query is flagged (needs_segmenter = 1) and gets no terms;
 *   AMDR_HAN_CHAR  text.jieba_cut_restated: blocks go through finalseg, one Han character per token;
 *   AMDR_HAN_DICT  text.dict_cut: jieba's default cut (prefix dictionary, word graph, maximum-log-probability route)
 *                  over the caller's dictionary, without the HMM — a run the dictionary does not cover comes out one Han
 *                  character per token.
 * In the last two modes encode / encode_joined / encode_ptrs (and a device copy made afterwards) cut such a query
 * themselves: flag 0, terms written.  A query without a Han character is cut as before in every mode.  Neither stand-in
 * is jieba.cut: the caller reports zh_exact = False for these queries.
 * set_han: call it before any encode and before amdr_tokenizer_device_create.  The dictionary is n_keys UTF-8 keys (key
 * i = key_blob[key_offsets[i] .. key_offsets[i+1]), non-empty): every word AND every proper prefix of a word, with
 * logw[i] = log(freq) - log(total) as the caller computed it (native code takes no logarithm: one fp64 add and one
 * compare per edge, so the route is the specification's bit for bit), is_word[i] = (freq > 0) and logw_unknown =
 * 0.0 - log(total).  Ignored unless mode is AMDR_HAN_DICT.  AMDR_EINVAL for a bad mode, a logw that is not finite, or
 * AMDR_HAN_DICT without keys (the handle is unchanged).
 * spans_han: amdr_tokenizer_spans for one text under the handle's mode (*n_tokens = -1: Han text under AMDR_HAN_FLAG). */
#define AMDR_HAN_FLAG 0
#define AMDR_HAN_CHAR 1
#define AMDR_HAN_DICT 2
int amdr_tokenizer_set_han(amdr_tokenizer_t* t, int32_t mode, const char* key_blob, const int64_t* key_offsets,
                           const double* logw, const uint8_t* is_word, int64_t n_keys, double logw_unknown);
int amdr_tokenizer_han_mode(const amdr_tokenizer_t* t, int32_t* mode);
int amdr_tokenizer_spans_han(const amdr_tokenizer_t* t, const char* text, int64_t n_bytes, int32_t* starts, int32_t* ends,
                             int32_t capacity, int32_t* n_tokens);
int amdr_tokenizer_destroy(amdr_tokenizer_t* t);
/* pack n queries that lie where they are (texts[q] = n_bytes[q] UTF-8 bytes; a Python caller takes the pointers from
 * the str objects themselves, csrc/pystrings.c) back to back into the caller's blob (e.g. pinned host memory, the source
 * of ONE host-to-device copy): offsets[nq + 1] with offsets[0] = 0, query q = blob[offsets[q] .. offsets[q + 1]).
 * AMDR_EINVAL when the bytes exceed capacity (nothing is copied).  Host code; the copies run on the tokeniser's pool. */
int amdr_tokenizer_pack(const char* const* texts, const int64_t* n_bytes, int32_t nq, char* blob, int64_t capacity,
                        int64_t* offsets);

/* ---- the same tokeniser on the device --------------------------------------
 * Replaces the same call site (legalrag/retrieval/bm25_retriever.py:73-74) as amdr_tokenizer_encode, with the query
 * texts already in HBM: writes the CSR amdr_bm25_search_device takes, byte for byte what amdr_tokenizer_encode writes
 * for the same blob (term_ids, q_ptr [nq+1] with q_ptr[0] = 0, needs_segmenter [nq]; a Han query: flag 1, no terms — or,
 * on a copy of a handle in AMDR_HAN_CHAR / AMDR_HAN_DICT, its terms and flag 0).
 * create: a device copy of a host tokeniser's vocabulary table (same hash, probe order, first id of a repeated term), of
 * its Han mode and of its dictionary table.
 * reserve: the largest batch (queries, bytes < 2^31) later calls take; the workspace is 16 bytes per byte of text, and 28
 * in AMDR_HAN_DICT (the route of a query: one double and one int32 per byte, in the query's own byte range).
 * encode_device: the blob text_dev[n_bytes] and offsets_dev[nq+1] are device pointers (query q = text_dev[offs[q] ..
 * offs[q+1]), ascending, <= n_bytes); term_ids_dev holds capacity entries and capacity >= n_bytes is required (tokens
 * <= bytes: it always suffices).  Only enqueues (4 launches on `stream`) and allocates nothing: capturable.  Returns
 * AMDR_EINVAL, and enqueues nothing, when capacity < n_bytes or the call exceeds the reserve.  Calls on one handle
 * share its workspace: order them (one stream). */
int amdr_tokenizer_device_create(const amdr_tokenizer_t* host, int32_t device, amdr_tokenizer_device_t** out);
int amdr_tokenizer_device_reserve(amdr_tokenizer_device_t* h, int32_t nq_max, int64_t bytes_max);
int amdr_tokenizer_encode_device(amdr_tokenizer_device_t* h, const char* text_dev, const int64_t* offs_dev, int32_t nq,
                                 int64_t n_bytes, int32_t* term_ids_dev, int64_t capacity, int64_t* q_ptr_dev,
                                 int32_t* needs_segmenter_dev, void* stream);
int amdr_tokenizer_device_destroy(amdr_tokenizer_device_t* h);

/* ---- ColBERT channel: exhaustive late-interaction MaxSim ---------------
 * Replaces `Searcher.search(query, k)` (legalrag/retrieval/colbert_retriever.py:152).
 * D: fp32 token embeddings [total_tokens, 128], doc_ptr[n_docs+1] (every doc
 * has >= 1 token); Q: [nq, 32, 128].  score = sum_i max_j <q_i, d_j>.
 * Arithmetic: every operand is split exactly into fp16 hi + lo / 2048 (22 significant bits) and a product is
 * hi*hi + (hi*lo + lo*hi) / 2048 on the fp16 matrix instructions with fp32 accumulation — scores within ~3e-6 of
 * the fp64 definition on unit-norm tokens (north_star's bar: 1e-4), scale-free for any finite input; a store
 * holding a NaN / infinity, or AMDR_MAXSIM_F16X3=0, takes the exact fp32-input matrix form (csrc/maxsim.hip).
 * Non-finite stores (fp32-input form; scores, search and search_device alike): a similarity <q_i, d_j> follows IEEE
 * arithmetic (a NaN component, inf x 0 or inf - inf make it NaN).  The maximum over a document's tokens starts at
 * -FLT_MAX and ignores a NaN similarity, so a -inf similarity never wins either and a +inf one does: a query token whose
 * similarities with a document are all NaN or -inf contributes -FLT_MAX, one with a +inf similarity +inf.  The
 * contributions are added in fp32: -FLT_MAX absorbs finite addends, two of them overflow to -inf.  Hence a NaN token
 * in a longer document drops out of it, a document of NaN tokens only scores -FLT_MAX (q_len == 1) or -inf, and no
 * score is ever NaN — the fp64 definition says NaN where this rule says a number.  (Only a document holding both
 * a +inf contribution and two -FLT_MAX ones has no defined score: inf - inf.)  In the top-k +inf ranks first and -inf
 * last, ahead of the -1 / -FLT_MAX padding, ties -> lower id as everywhere.  Every other document keeps the bits it
 * has in the same store with the non-finite token replaced by zeros.  Tested in tests/test_maxsim_adversary_gpu.py. */
int amdr_maxsim_create(const float* D_host, const int64_t* doc_ptr, int64_t n_docs, int32_t dim,
                       int32_t device, amdr_maxsim_t** out);
/* Append n_add documents (replaces re-running the indexer over the whole corpus, legalrag/retrieval/builders/
 * colbert_builder.py:131-132, for an ingest): D_host fp32 [doc_ptr_add[n_add], 128], doc_ptr_add[0] == 0, strictly ascending
 * (every document >= 1 token); new pids are n_docs .. n_docs + n_add - 1.  Afterwards the handle is what
 * amdr_maxsim_create makes of the concatenated store: the same scale, first-pass bound and image bytes, hence the same
 * ids and score bits from every entry point.  The new rows' largest |component| joins the store's; the images of the
 * old rows stay as they are unless that raises the store's power-of-two scale (then the whole store is converted
 * again); new rows holding a NaN / infinity drop the images (fp32-input form from then on, as after such a create).
 * Storage doubles, or grows to fit.  AMDR_EINVAL: null handle, n_add < 0, null pointers with n_add > 0,
 * doc_ptr_add[0] != 0, an empty document, n_docs + n_add >= 2^32; n_add == 0 is a no-op.  A failed add (AMDR_ENOMEM,
 * AMDR_EHIP) leaves the handle as it was and searchable.  The price of that: an add that has to grow the storage, or
 * to convert the store again, holds the old and the new copy of what it replaces (D, img and img_hi: 4 + 4 + 2 bytes
 * per component) until it has succeeded — up to twice the steady state for the length of the call, so it can return
 * AMDR_ENOMEM on a device where the store itself fits; an add within the capacity at an unchanged scale allocates nothing.
 * Runs inside the handle's mutex: host-pointer searches from other threads serialise against it.  It is a mutation in
 * the sense of the rule at the top of this file: "_device" work of the handle still in flight is the caller's to finish
 * first (buffers it reads may be freed).  Workspaces are sized per call from n_docs: an eager "_device" call after an add
 * grows its workspace if it has to (amdr_workspace_growths shows it); a captured graph holds the old buffers and sizes
 * and must be re-reserved (amdr_maxsim_reserve) and captured again. */
int amdr_maxsim_add(amdr_maxsim_t* h, const float* D_host, const int64_t* doc_ptr_add, int64_t n_add);
/* Remove n_remove documents (the reference has no removal: a corpus that shrinks takes the indexer over everything
 * again, legalrag/retrieval/builders/colbert_builder.py:131-132, and then the reload of
 * legalrag/retrieval/colbert_retriever.py, which this call replaces).  remove_ids[n_remove]: old pids, strictly
 * ascending, in [0, n_docs); n_remove < n_docs (a store keeps a document, as create demands).  The surviving documents
 * are renumbered 0 .. n_docs-n_remove-1 in their old order and their token rows close up.
 * Afterwards the handle is what amdr_maxsim_create makes of the surviving store: D and doc_ptr are the same bytes
 * (amdr_maxsim_read), and create's own sequence runs on the new D — largest |component|, power-of-two scale, both images
 * converted again from D (fewer bytes per token than copying them, and create's bytes by construction), d_norm_max —
 * hence the same ids and score bits from every entry point.  Unlike under add the scale and d_norm_max can FALL; a store
 * that had no images gets them when its last NaN / infinity is removed; info[5] goes up by one per remove of a store
 * that is finite afterwards.  The work: two small kernels rebuild doc_ptr, one ordered compaction moves the 512-byte
 * token rows at HBM speed into a NEW buffer (csrc/rows_compact.hip; no atomics, deterministic), then the conversion.
 * Capacity afterwards equals the survivors; a later add grows as it does today.
 * AMDR_EINVAL: null handle, n_remove < 0, null remove_ids, n_remove >= n_docs, an id outside [0, n_docs), ids not
 * strictly ascending.  n_remove == 0 is a no-op that reads nothing.  A failed remove (AMDR_EINVAL, AMDR_ENOMEM, AMDR_EHIP)
 * leaves the handle as it was and searchable.  The price of that: the old and the new copy of D, doc_ptr and both images
 * (4 + 4 + 2 bytes per component) plus 16 B per surviving document and 8 B per removed id of scratch are resident for the
 * length of the call, so it can return AMDR_ENOMEM on a device where the store itself fits.  Runs inside the handle's
 * mutex.  It is a mutation in the sense of the rule at the top of this file, and the rules for in-flight "_device" work,
 * for workspaces (never shrunk) and for captured graphs are those of amdr_maxsim_add: finish the work first, reserve and
 * capture again.  Pids held by others (scope tables, pid -> chunk maps) are the caller's to rebuild. */
int amdr_maxsim_remove(amdr_maxsim_t* h, const int64_t* remove_ids, int64_t n_remove);
/* Summed device time of the doc_ptr rebuild and the compaction kernel of the last successful amdr_maxsim_remove, in ms
 * between events on the handle's stream (scripts/bench_store_remove.py); -1 before the first remove. */
int amdr_maxsim_remove_kernel_ms(amdr_maxsim_t* h, double* ms);
/* Replace n_rep documents under their pids (the reference has no update: an amended passage takes the indexer over
 * everything again, legalrag/retrieval/builders/colbert_builder.py:131-132).  replace_ids[n_rep]: old pids, strictly
 * ascending, in [0, n_docs); document replace_ids[i] takes the token rows D_host[doc_ptr_add[i] .. doc_ptr_add[i + 1])
 * (doc_ptr_add[0] == 0, every document has >= 1 token; a document may grow, shrink or keep its length).  No pid moves.
 * Afterwards the handle is what amdr_maxsim_create makes of the edited store: D and doc_ptr are the same bytes
 * (amdr_maxsim_read), and create's own sequence has run on the new D — largest |component|, power-of-two scale, both
 * images converted again, d_norm_max — hence the same ids and score bits from every entry point.  As under remove the
 * scale and d_norm_max can FALL, a store whose last NaN / infinity is replaced away gets its images, and info[5] goes up
 * by one per replace of a store that is finite afterwards.  The work: the new rows, their doc_ptr and the ids are staged
 * on the device, two small kernels rebuild doc_ptr (lengths, then the scan), one ordered splice writes the 512-byte token
 * rows in 16-byte units into a NEW buffer, each from the old D or from the staged rows (csrc/rows_compact.hip; no
 * atomics, deterministic), then the conversion.  Capacity afterwards equals the store.
 * AMDR_EINVAL: null handle, n_rep < 0, null replace_ids / D_host / doc_ptr_add, n_rep > n_docs, an id outside
 * [0, n_docs), ids not strictly ascending, doc_ptr_add[0] != 0, a document without tokens.  n_rep == 0 is a no-op that
 * reads nothing.  A failed replace (AMDR_EINVAL, AMDR_ENOMEM, AMDR_EHIP) leaves the handle as it was and searchable.
 * Transient memory: the old and the new copy of D, doc_ptr and both images (4 + 4 + 2 bytes per component), the staged
 * rows (512 B per new token, 8 B per replaced document) and 16 B per document of scratch are resident for the length of
 * the call, so it can return AMDR_ENOMEM on a device where the store itself fits.  Runs inside the handle's mutex.  It is
 * a mutation in the sense of the rule at the top of this file, and the rules for in-flight "_device" work and for
 * captured graphs are those of amdr_maxsim_add: finish the work first, reserve and capture again. */
int amdr_maxsim_replace(amdr_maxsim_t* h, const int64_t* replace_ids, const float* D_host, const int64_t* doc_ptr_add,
                        int64_t n_rep);
/* Summed device time of the doc_ptr rebuild and the splice kernel of the last successful amdr_maxsim_replace, in ms
 * between events on the handle's stream (scripts/bench_replace.py); -1 before the first replace. */
int amdr_maxsim_replace_kernel_ms(amdr_maxsim_t* h, double* ms);
/* Copies the resident store to the host: D [n_tokens, 128], doc_ptr [n_docs + 1] (sizes from amdr_maxsim_info); either
 * pointer may be null.  Synchronous, inside the handle's mutex.  The only way to see what a handle holds. */
int amdr_maxsim_read(amdr_maxsim_t* h, float* D_host, int64_t* doc_ptr_host);
/* out6: [0] n_docs, [1] n_tokens, [2] token capacity, [3] e of d_scale = 2^e, [4] 1 if the split-fp16 images exist,
 *       [5] whole-store conversions so far (amdr_maxsim_create of a finite store counts 1) */
int amdr_maxsim_info(amdr_maxsim_t* h, int64_t* out6);
/* The two numbers of the store that the bound of the two-pass top-k's first pass is built on: out2[0] = d_scale (a power
 * of two; 1 for a store without images), out2[1] = d_norm_max, the largest token L2 norm of the store x d_scale (0 without
 * images).  After any sequence of adds both have the bits amdr_maxsim_create gives them on the concatenated store. */
int amdr_maxsim_stats(amdr_maxsim_t* h, float* out2);
int amdr_maxsim_ndocs(const amdr_maxsim_t* h, int64_t* n);
/* which kernels a search of nq queries would launch and in which arithmetic form (NUL-terminated; no device work) */
int amdr_maxsim_plan_info(const amdr_maxsim_t* h, int32_t nq, char* buf, int32_t buf_len);
int amdr_maxsim_reserve(amdr_maxsim_t* h, int32_t nq_max, int32_t k_max);
/* Host-only: the same for MaxSim on n_docs documents, split_image = 1 when the store has its split-fp16 images (every
 * finite store; the two-pass top-k needs them): out2[0] = the workspace bytes amdr_maxsim_reserve(nq_max, k_max) sizes,
 * out2[1] = the bytes amdr_maxsim_search_device(nq, k) uses (both follow AMDR_MAXSIM_F16X3 / AMDR_MAXSIM_TWOPASS).
 * A one-pass call uses its score rows [nq, n_docs], rounded up to 256 bytes; for a two-pass call out2[1] is the exact
 * end of the layout the call runs in (a multiple of 256), not an upper bound, and the call checks it against the
 * workspace it is given. */
int amdr_maxsim_workspace_plan(int64_t n_docs, int32_t split_image, int32_t nq_max, int32_t k_max, int32_t nq, int32_t k,
                               int64_t* out2);
int amdr_maxsim_search(amdr_maxsim_t* h, const float* Q_host, int32_t nq, int32_t q_len, int32_t k,
                       float* scores_host, int64_t* ids_host);
int amdr_maxsim_search_device(amdr_maxsim_t* h, const float* Q_dev, int32_t nq, int32_t q_len, int32_t k,
                              float* scores_dev, int64_t* ids_dev, void* stream);
int amdr_maxsim_scores(amdr_maxsim_t* h, const float* Q_host, int32_t nq, int32_t q_len, float* scores_host);
int amdr_maxsim_destroy(amdr_maxsim_t* h);

/* ---- fusion + rerank blend ---------------------------------------------
 * Replaces HybridRetriever._fuse (legalrag/retrieval/hybrid_retriever.py:389-551)
 * with its helpers _minmax (:24-30) and _rrf_with_breakdown (:33-56), the
 * min_final_score filter (:309-310) and the rerank blend (:338-355 with
 * rerankers.py:48-54,349).  float64, no FMA contraction: bit-identical to the
 * Python float arithmetic.  Exactly tied fused scores keep first-appearance
 * order (dense list, then bm25, then colbert). */
#define AMDR_FUSE_RRF_NORM_BLEND 0
#define AMDR_FUSE_RRF 1
#define AMDR_FUSE_WRRF 2
#define AMDR_FUSE_WEIGHTED_SUM 3

typedef struct amdr_fuse_params {
  int32_t method;          /* AMDR_FUSE_* */
  int32_t rrf_k;           /* cfg.retrieval.rrf_k (60) */
  double alpha;            /* cfg.retrieval.rrf_alpha (0.5) */
  double w_dense, w_bm25, w_colbert;
  double min_final_score;  /* drop fused hits below this; -inf keeps all */
} amdr_fuse_params_t;

/* values per fused candidate, AMDR_FUSE_NVALS doubles each */
#define AMDR_FUSE_NVALS 9
#define AMDR_FV_SCORE 0
#define AMDR_FV_RRF_NORM 1
#define AMDR_FV_WSUM 2
#define AMDR_FV_NORM_DENSE 3
#define AMDR_FV_NORM_BM25 4
#define AMDR_FV_NORM_COLBERT 5
#define AMDR_FV_CONTRIB_DENSE 6
#define AMDR_FV_CONTRIB_BM25 7
#define AMDR_FV_CONTRIB_COLBERT 8

/* Inputs per channel: ids [nq, k_c] (-1 = padding, valid entries first, sorted
 * by score descending), scores [nq, k_c]; a channel with k_c == 0 is absent.
 * *_row2uid (nullable) maps a channel's row id to the corpus-wide chunk uid.
 * Outputs, max_out = kd+kb+kc entries per query, in fused-rank order:
 * out_ids [nq,max_out], out_vals [nq,max_out,AMDR_FUSE_NVALS], out_mask
 * [nq,max_out] (bit0 dense, bit1 bm25, bit2 colbert membership), out_count
 * [nq] = hits surviving the min_final_score filter. */
/* host-pointer form: every channel's scores as double (callers of _fuse may
 * hand in arbitrary Python floats; fp32 channel scores widen exactly) */
int amdr_fuse(const amdr_fuse_params_t* p, int32_t nq,
              const int64_t* dense_ids, const double* dense_scores, int32_t kd,
              const int64_t* bm25_ids, const double* bm25_scores, int32_t kb,
              const int64_t* colbert_ids, const double* colbert_scores, int32_t kc,
              int64_t* out_ids, double* out_vals, int32_t* out_mask, int32_t* out_count);
int amdr_fuse_device(const amdr_fuse_params_t* p, int32_t nq,
                     const int64_t* dense_ids, const float* dense_scores, int32_t kd, const int64_t* dense_row2uid,
                     const int64_t* bm25_ids, const double* bm25_scores, int32_t kb, const int64_t* bm25_row2uid,
                     const int64_t* colbert_ids, const float* colbert_scores, int32_t kc, const int64_t* colbert_row2uid,
                     int64_t* out_ids, double* out_vals, int32_t* out_mask, int32_t* out_count,
                     int32_t device, void* stream);

/* amdr_dense_search_device followed by amdr_fuse_device(dense lists, BM25 lists, no ColBERT) as ONE call — the same
 * outputs, bit for bit (dense_scores / dense_ids: the dense channel's own top-k; out_*: the fusion's), fewer launches:
 * for the serving corpora under a batch (<= 1 024 rows, k + kb <= 32) the rows are ranked and fused by one kernel
 * (two queries per wave), every other shape runs the two launches inside.  Reference stages:
 * hybrid_retriever.py:181-189 (search_dense) + :389-551 (_fuse).  AMDR_DENSE_FUSE=0 pins the two launches. */
int amdr_dense_search_fuse_device(amdr_dense_t* h, const float* Q_dev, int32_t nq, int32_t k,
                                  const amdr_fuse_params_t* p, const int64_t* dense_row2uid,
                                  const int64_t* bm25_ids, const double* bm25_scores, int32_t kb,
                                  const int64_t* bm25_row2uid, float* dense_scores_dev, int64_t* dense_ids_dev,
                                  int64_t* out_ids, double* out_vals, int32_t* out_mask, int32_t* out_count,
                                  void* stream);

/* The serving call — HybridRetriever.search(), one query at a time (hybrid_retriever.py:282-384: search_dense :181-189,
 * search_bm25 :191-209, _fuse :389-551) — as ONE launch: amdr_bm25_search_device + amdr_dense_search_fuse_device, the same
 * five outputs bit for bit (bm25_scores/ids [nq,kb], dense_scores/ids [nq,kd], out_* as amdr_fuse_device), for 1-4
 * queries on a corpus of <= 2 048 chunks held by both indexes on the same device with kd + kb <= 32: blocks of the one
 * grid score the BM25 slab or 4-16 chunk rows each, and the last block of a query to arrive ranks and fuses.  Every other
 * shape (and AMDR_HYBRID_SMALL=0) runs the two calls inside.  Only enqueues; after amdr_dense_reserve + amdr_bm25_reserve
 * it allocates nothing (capturable).  One call at a time per pair of handles (they share the handles' workspaces). */
int amdr_hybrid_small_device(amdr_dense_t* dense, amdr_bm25_t* bm25, const float* Q_dev, const int32_t* q_terms_dev,
                             const int64_t* q_ptr_dev, int32_t nq, int32_t kd, int32_t kb, const amdr_fuse_params_t* p,
                             const int64_t* dense_row2uid, const int64_t* bm25_row2uid, float* dense_scores_dev,
                             int64_t* dense_ids_dev, double* bm25_scores_dev, int64_t* bm25_ids_dev, int64_t* out_ids,
                             double* out_vals, int32_t* out_mask, int32_t* out_count, void* stream);

/* The long-batch hybrid step — HybridRetriever.search_batch on dense + BM25 (hybrid_retriever.py: search_dense :181-189,
 * search_bm25 :191-209, _fuse :389-551) — as ONE call: amdr_bm25_search_device + amdr_dense_search_fuse_device, the same
 * five outputs bit for bit (arguments as amdr_hybrid_small_device).  Where the dense channel takes its two-pass form as
 * one pass (from 4 096 queries on <= 1 024 rows, d a multiple of 128, kd <= 12, kd + kb <= 32) and both indexes are on
 * the same device, the call forks inside, behind the first pass's scores kernel: BM25 runs on the dense handle's side
 * stream beside the second dense pass on the caller's stream, and the fusion runs behind the join.  Fork and join are events: the caller's stream is ordered
 * behind both branches when the call returns (the next call may reuse the workspaces), and while the caller's stream is
 * capturing they become graph edges.  Every other shape, and AMDR_HYBRID_BATCH=0, runs the two calls inside.  Only
 * enqueues; the side stream and its events are made by amdr_dense_create / amdr_dense_reserve, and after
 * amdr_dense_reserve + amdr_bm25_reserve the call allocates nothing (capturable).  One call at a time per pair of handles. */
int amdr_hybrid_batch_device(amdr_dense_t* dense, amdr_bm25_t* bm25, const float* Q_dev, const int32_t* q_terms_dev,
                             const int64_t* q_ptr_dev, int32_t nq, int32_t kd, int32_t kb, const amdr_fuse_params_t* p,
                             const int64_t* dense_row2uid, const int64_t* bm25_row2uid, float* dense_scores_dev,
                             int64_t* dense_ids_dev, double* bm25_scores_dev, int64_t* bm25_ids_dev, int64_t* out_ids,
                             double* out_vals, int32_t* out_mask, int32_t* out_count, void* stream);

/* The first pass of the two-pass form of the long-batch dense channel on a short corpus (search_dense over a batch,
 * hybrid_retriever.py:181-189) — what amdr_dense_search_device / amdr_dense_search_fuse_device run inside from 4 096
 * queries per launch on <= 1 024 rows with d a multiple of 128 and k <= 12 (AMDR_DENSE_SMALL_HI=0: the
 * exact fp32 form), exported for tests and measurements.  approx_device writes, for every
 * query and chunk row, the dot product of the fp16 roundings of the scaled operands — S[nq, ldS] (ldS >= the rows padded to
 * 32, a multiple of 4; columns [n, padded) are 0) — on the fp16 matrix instructions, and per query the PROVEN bound
 * eps[q] >= |S[q][r] - <Q[q], X[r]>| for every row r (NaN: a non-finite query or one outside the scale range — no bound),
 * in the units of the exact score.  The second pass (inside the search calls) re-scores the rows with
 * S >= (k-th best of S) - 2 eps in exact fp32 and ranks them: the exact top-k, ties to the lower row.  create takes the statistics and the fp16 image of the dense handle's matrix as it is NOW (rows added
 * later are not seen); d must be a multiple of 128 in [128, 1024]; the dense handle must outlive this one. */
/* queries of this handle's two-pass searches so far that re-scored their WHOLE row inside the second pass (more than 32 rows
 * inside the margin, or no bound for the query): the results are exact either way, a large share means the data does not suit
 * the form (AMDR_DENSE_SMALL_HI=0).  Synchronises with the device. */
int amdr_dense_two_pass_fallbacks(amdr_dense_t* h, int64_t* out);
int amdr_dense_small_create(amdr_dense_t* dense, amdr_dense_small_t** out);
int amdr_dense_small_approx_device(amdr_dense_small_t* h, const float* Q_dev, int32_t nq, float* S_dev, int64_t ldS,
                                   float* eps_dev /* nullable [nq] */, void* stream);
int amdr_dense_small_destroy(amdr_dense_small_t* h);

/* Rerank blend over the first min(top_n, count[q]) fused hits of each query:
 * norm = minmax(ce_raw); score = (1-beta)*score + beta*norm; the candidates
 * are re-ordered by norm (stable), written back in front of the rest, and the
 * whole list is stably re-sorted by the new score.  In place on ids/vals/mask;
 * out_rerank [nq,max_out,2] receives (raw, norm) per OUTPUT position, NaN for
 * hits that were not reranked. ce_raw: [nq, top_n]. */
int amdr_rerank_blend(int32_t nq, int32_t max_out, const int32_t* count, int64_t* ids, double* vals,
                      int32_t* mask, const double* ce_raw, int32_t top_n, double beta, double* out_rerank);
int amdr_rerank_blend_device(int32_t nq, int32_t max_out, const int32_t* count, int64_t* ids, double* vals,
                             int32_t* mask, const double* ce_raw, int32_t top_n, double beta,
                             double* out_rerank, int32_t device, void* stream);

/* The columns a bulk caller reads from a fused result, compacted on the device: the first w fused hits of every query
 * as out_rows / out_scores / out_mask [nq, w] (entries past min(count[q], w): -1 / 0.0 / 0) and out_count [nq] =
 * min(count[q], w).  Inputs: the outputs of amdr_fuse_device (after the optional rerank blend).  One small device-to-host
 * copy then serves HybridRetriever.search_batch_arrays (hybrid_retriever.py:309-310 + :384, the cut to top_k). */
int amdr_fuse_compact_device(int32_t nq, int32_t max_out, int32_t w, const int64_t* ids, const double* vals,
                             const int32_t* mask, const int32_t* count, int64_t* out_rows, double* out_scores,
                             int32_t* out_mask, int32_t* out_count, int32_t device, void* stream);

/* ---- diversification: maximal-marginal-relevance (MMR) selection over the resident chunk matrix -------------------
 * Picks k_sel of a query's first `pool` fused hits, trading relevance against similarity to the hits already picked
 * (Carbonell & Goldstein 1998).  The reference has no such stage and no call site for it: this is the project's own, as
 * scoped search is.  One block per query; no workspace, no atomics, deterministic (csrc/mmr.hip).
 *
 * Per query q:  m = min(max(count[q], 0), pool);  rows[q][0..m) are rows of `dense` in fused-rank order
 * (rows + q*ld_rows);  rel[q][i] is the double at rel + q*rel_ld + i*rel_stride (a packed fused result: rel_stride =
 * AMDR_FUSE_NVALS, rel_ld = max_out*AMDR_FUSE_NVALS, rel pointing at AMDR_FV_SCORE; a plain matrix: 1, ld).
 *   Gram:    G[i][j] = the fp32 inner product of X[rows[i]] and X[rows[j]] (summation order unspecified); ONE value
 *            serves (i, j) and (j, i).  A candidate whose row is < 0 or >= n has no vector: its G row and column are 0.
 *   cosine:  cos[i][j] = (double)G[i][j] / sqrt((double)G[i][i] * (double)G[j][j]) in fp64, no contraction; 0 when the
 *            denominator is not finite and > 0, or G[i][j] is not finite.
 *   greedy:  min(k_sel, m) steps.  maxsim[i] = the maximum of cos[i][j] over the j selected so far, 0.0 while there is
 *            none;  mmr[i] = lambda * rel[i] - (1.0 - lambda) * maxsim[i] (two fp64 products, one subtraction).  A step
 *            selects the unselected i of the largest mmr[i]; ties go to the lower i; a NaN ranks behind every number
 *            (-inf included) and NaNs keep position order.
 * Outputs [nq, k_sel], in selection order: out_pos (the position i; -1 past out_count[q]), out_mmr (the winning value;
 * 0.0), out_maxsim (its maxsim when it was selected; 0.0); out_count [nq] = min(k_sel, m).
 * Errors (AMDR_EINVAL): a null pointer, pool outside [1, AMDR_MMR_MAX_POOL], k_sel outside [1, pool], lambda outside
 * [0, 1] or NaN, ld_rows < pool, nq < 0, rel_stride < 1 or rel_ld < 0.  nq == 0 succeeds and does nothing.
 * amdr_mmr_device only enqueues on `stream` (capturable, no reserve call); amdr_mmr takes host pointers, runs on the
 * handle's own stream under its mutex and synchronises. */
#define AMDR_MMR_MAX_POOL 64
int amdr_mmr_device(amdr_dense_t* dense, const int64_t* rows_dev, int32_t ld_rows, const double* rel_dev,
                    int64_t rel_stride, int64_t rel_ld, const int32_t* count_dev, int32_t nq, int32_t pool, int32_t k_sel,
                    double lambda, int32_t* out_pos, double* out_mmr, double* out_maxsim, int32_t* out_count, void* stream);
int amdr_mmr(amdr_dense_t* dense, const int64_t* rows_host, int32_t ld_rows, const double* rel_host, int64_t rel_stride,
             int64_t rel_ld, const int32_t* count_host, int32_t nq, int32_t pool, int32_t k_sel, double lambda,
             int32_t* out_pos, double* out_mmr, double* out_maxsim, int32_t* out_count);

/* ---- graph channel: law-graph walk + re-scoring of the walked articles --------------------------------------------
 * Replaces, for a whole batch, the per-query host stage HybridRetriever.search runs for a GRAPH_AUGMENTED decision
 * (legalrag/retrieval/hybrid_retriever.py:312-322): LawGraphStore.walk (graph_store.py:89-169, a Python BFS over up to
 * graph_limit nodes), the re-embedding of every visited article and its cosine with the query, the score product and
 * the sort (graph_retriever.py:82-219).  csrc/graph.hip.
 * Graph tables (host arrays, copied to the device at creation), over n_nodes interned article ids:
 *   node_ptr i64 [n_nodes + 1], edge_dst i32 / edge_rel i32 / edge_conf_raw f64 / edge_conf_eff f64 /
 *   edge_has_evidence i32 [n_edges]   CSR adjacency in file order; conf_raw = float(conf or 1.0) (the min_conf filter),
 *                                     conf_eff = the edge confidence the score takes (conf_raw with evidence, else the
 *                                     stored destination's meta "_edge_conf" or 1.0)
 *   node_present i32 [n_nodes]        1 = a stored node (found and expanded); 0 = a destination only (claimed, never
 *                                     emitted), as on the host
 *   node_row i64 [n_nodes]            chunk row of the node's article (-1: no chunk, empty text)
 *   row_node i32 [n_rows]             node of the stripped article key of a chunk row (-1: none)
 *   row_norm f32 [n_rows]             row L2 norms as the host computes them; row_lang i32 [n_rows] (nullable)
 * Per call (amdr_graph_params_t): limit in [1, 4096] found nodes, default_depth (seeds), min_conf (> 0: edges with
 * conf_raw below it are skipped), per relation max_depth (a node reached by relation r expands while its depth <
 * max_depth[r]), allowed (0/1) and weight, decay[0 .. limit] (decay[depth]), lang (-1 = any; else rows whose row_lang
 * differs drop out).  The tables are HOST pointers for amdr_graph_walk / amdr_graph_search and DEVICE pointers for
 * amdr_graph_search_device.
 * Per query: seeds = the first min(seed_n <= 1024, seed_count[q]) entries of row q of seeds [*, ld]; the walk equals
 * LawGraphStore.walk node for node; every found node with a chunk row scores
 *   semantic = <q, X[row]> / (sqrtf(<q, q>) * row_norm[row] + 1e-9f)   (fp32; the dot as amdr_dense_score_rows)
 *   final    = ((double)semantic * decay[depth]) * weight[rel] * conf_eff
 * and the top k <= AMDR_MAX_K by final are written, ties -> earlier walk position: out_count [n], out_rows i64,
 * out_final f64, out_semantic f32, out_depth i32, out_rel i32, out_conf f64 (conf_eff) [n, k] (past out_count: -1 /
 * 0).  Non-finite scores: a NaN final ranks behind every number (-inf included), NaN entries in walk order among
 * themselves; +-inf order as numbers.  Every valid found node appears exactly once and out_count = min(valid, k).
 * The only difference from the host path: numpy computes |q| with BLAS in its own summation order.
 * The dense handle gives the resident chunk matrix (same device; its rows are the chunk rows above). */
typedef struct amdr_graph_params {
  int32_t limit;
  int32_t default_depth;
  int32_t lang;
  int32_t pad0;
  double min_conf;
  const int32_t* rel_max_depth;
  const int32_t* rel_allowed;
  const double* rel_weight;
  const double* decay;
} amdr_graph_params_t;
int amdr_graph_create(const int64_t* node_ptr, const int32_t* edge_dst, const int32_t* edge_rel,
                      const double* edge_conf_raw, const double* edge_conf_eff, const int32_t* edge_has_evidence,
                      const int32_t* node_present, const int64_t* node_row, const int32_t* row_node,
                      const float* row_norm, const int32_t* row_lang, int32_t n_nodes, int64_t n_edges,
                      int64_t n_rows, int32_t n_rel, int32_t device, amdr_graph_t** out);
/* sizes the "_device" workspace: up to nq_max queries per call, k <= k_max, limit <= limit_max */
int amdr_graph_reserve(amdr_graph_t* h, int32_t nq_max, int32_t k_max, int32_t limit_max);
/* the walk alone (host pointers; seeds are NODE ids here): per query out_count [nq] and, in found order, out_node /
 * out_depth / out_parent / out_rel / out_evidence (edge_has_evidence) i32 and out_conf (edge_conf_raw) f64 [nq, limit]
 * (past out_count: -1 / 0).  LawGraphStore.walk (graph_store.py:89-169); the hook the walk tests use. */
int amdr_graph_walk(amdr_graph_t* h, const int64_t* seeds_host, const int32_t* seed_count_host, int32_t ld,
                    int32_t seed_n, int32_t nq, const amdr_graph_params_t* params, int32_t* out_count,
                    int32_t* out_node, int32_t* out_depth, int32_t* out_parent, int32_t* out_rel, int32_t* out_evidence,
                    double* out_conf);
/* walk + re-scoring + top-k from host query vectors Q [nq, d] and seed CHUNK rows [nq, ld] (GraphRetriever.search,
 * graph_retriever.py:82-219) */
int amdr_graph_search(amdr_graph_t* h, amdr_dense_t* dense, const float* Q_host, const int64_t* seeds_host,
                      const int32_t* seed_count_host, int32_t ld, int32_t seed_n, int32_t nq, int32_t k,
                      const amdr_graph_params_t* params, int32_t* out_count, int64_t* out_rows, double* out_final,
                      float* out_semantic, int32_t* out_depth, int32_t* out_rel, double* out_conf);
/* the same on device pointers, enqueued on `stream` (capturable after amdr_graph_reserve): for g < ng the query row
 * q = qsel[g] (qsel nullable: q = g) of Q [*, d], seeds [*, ld] (e.g. BatchResult ids, the fused list) and seed_count
 * [*] (its count); outputs indexed by g.  Replaces the per-query loop of HybridRetriever.search_batch over the
 * graph-mode queries (hybrid_retriever.py:312-322 once per query: walk, store._embed(question), score, sort). */
int amdr_graph_search_device(amdr_graph_t* h, amdr_dense_t* dense, const float* Q_dev, const int32_t* qsel_dev,
                             const int64_t* seeds_dev, const int32_t* seed_count_dev, int32_t ld, int32_t seed_n,
                             int32_t ng, int32_t k, const amdr_graph_params_t* params, int32_t* out_count,
                             int64_t* out_rows, double* out_final, float* out_semantic, int32_t* out_depth,
                             int32_t* out_rel, double* out_conf, void* stream);
int amdr_graph_destroy(amdr_graph_t* h);

/* ---- scoped search: the top-k of a query's OWN rows in the dense, BM25 and ColBERT channels ------------------------
 * No reference counterpart: HybridRetriever.search (legalrag/retrieval/hybrid_retriever.py:282-384) ranks the whole corpus
 * and has no scope argument; a caller who asks "within this chapter" over-fetches and filters on the host.  csrc/scope.hip.
 * A scope is an ascending list of rows of ONE channel's row space (dense rows, BM25 documents and ColBERT documents each
 * have their own).  The table travels with each call: scope_ptr i64 [n_scopes + 1] indexes rows i64 [...], qscope i32 [nq]
 * names each query's scope, rows_max = the longest scope of the call (the grid is sized from it; rows past it are not
 * ranked).  Per query the top k <= AMDR_MAX_K of its scope's rows, by the score the unscoped channel gives each row — bit
 * for bit (dense: amdr_dense_score_rows; BM25: amdr_bm25_scores, idf and avgdl of the WHOLE index; MaxSim: the split-fp16
 * pair form of amdr_maxsim_scores, the store's scale) — with the channel's own order: score descending, ties -> lower id,
 * NaN last, -0.0 as +0.0, BM25 zero-score documents returned; padding id -1 / -FLT_MAX (-DBL_MAX) behind a scope shorter
 * than k.  An empty scope or a qscope outside [0, n_scopes) gives an all-padding list and reads nothing; a row outside
 * [0, n) is skipped and never dereferenced.  Work is proportional to the scopes, not to the corpus.
 * amdr_scope_t is a workspace holder and owns no table: one region of slab lists per channel, so the three "_device"
 * calls of a step need no ordering among themselves (calls of the SAME channel on one handle share its region: order
 * them).  reserve: the largest call (queries, depth, longest scope); a scope inside one slab of rows needs no workspace.
 * AMDR_SCOPE_SLAB=<rows> pins the slab length of all three channels (<= 1 024; read per call and by reserve /
 * workspace_plan: set it before the reserve).
 * The "_device" calls take the channel's handle, the query operand in the channel's own device form and the table as
 * device pointers; they only enqueue on `stream` (one launch, plus the merge when a scope spans slabs), allocate nothing
 * and return AMDR_EINVAL, enqueueing nothing, when the call exceeds the reserve.  amdr_scope_maxsim_* return AMDR_EINVAL
 * for a store without its split-fp16 image and under AMDR_MAXSIM_F16X3=0.
 * The host-pointer twins validate the table (AMDR_EINVAL: scope_ptr not monotone, a scope's rows not strictly ascending
 * or outside [0, n)), stage it, run on the scope handle's own stream and return after the lists are in the host buffers. */
int amdr_scope_create(int32_t device, amdr_scope_t** out);
int amdr_scope_reserve(amdr_scope_t* h, int32_t nq_max, int32_t k_max, int64_t rows_max);
/* Host-only (no device is touched): out6[0..2] = the bytes amdr_scope_reserve(nq_max, k_max, rows_max_reserve) sizes for
 * the dense / BM25 / MaxSim region, out6[3..5] = the bytes a "_device" call (nq, k, rows_max) uses of each.  A test holds
 * out6[3+i] <= out6[i] for every nq <= nq_max, k <= k_max, rows_max <= rows_max_reserve (tests/test_scope.py). */
int amdr_scope_workspace_plan(int32_t nq_max, int32_t k_max, int64_t rows_max_reserve, int32_t nq, int32_t k,
                              int64_t rows_max, int64_t* out6);
/* which kernels the three scoped calls of (nq, k, rows_max) would launch, how a scope is cut into slabs, and whether the
 * step of dense + BM25 at depth k each (amdr_hybrid_scope_device) is the one launch of scope_hybrid_kernel
 * (NUL-terminated; no device work) */
int amdr_scope_plan_info(const amdr_scope_t* h, int32_t nq, int32_t k, int64_t rows_max, char* buf, int32_t buf_len);
int amdr_scope_dense_search_device(amdr_scope_t* h, amdr_dense_t* dense, const float* Q_dev, const int64_t* scope_ptr_dev,
                                   const int64_t* rows_dev, const int32_t* qscope_dev, int32_t n_scopes, int64_t rows_max,
                                   int32_t nq, int32_t k, float* scores_dev, int64_t* ids_dev, void* stream);
int amdr_scope_bm25_search_device(amdr_scope_t* h, amdr_bm25_t* bm25, const int32_t* q_terms_dev, const int64_t* q_ptr_dev,
                                  const int64_t* scope_ptr_dev, const int64_t* rows_dev, const int32_t* qscope_dev,
                                  int32_t n_scopes, int64_t rows_max, int32_t nq, int32_t k, double* scores_dev,
                                  int64_t* ids_dev, void* stream);
int amdr_scope_maxsim_search_device(amdr_scope_t* h, amdr_maxsim_t* maxsim, const float* Q_dev, int32_t q_len,
                                    const int64_t* scope_ptr_dev, const int64_t* rows_dev, const int32_t* qscope_dev,
                                    int32_t n_scopes, int64_t rows_max, int32_t nq, int32_t k, float* scores_dev,
                                    int64_t* ids_dev, void* stream);
/* The scoped STEP — dense + BM25 top-k of each query's own rows, then the fusion — as one call.  No reference counterpart
 * (legalrag/retrieval/hybrid_retriever.py:282-384 has no scope argument); it computes what amdr_scope_dense_search_device,
 * amdr_scope_bm25_search_device and amdr_fuse_device compute from the same arguments, bit for bit: the two channel lists
 * (dense_scores f32 / dense_ids [nq, kd], bm25_scores f64 / bm25_ids [nq, kb]) and the fused record (out_ids [nq, mo],
 * out_vals [nq, mo, AMDR_FUSE_NVALS], out_mask [nq, mo], out_count [nq], mo = kd + kb + kc).  The dense and the BM25 scope
 * come from their own tables (d_* / b_*: their row spaces differ); ids are mapped through each channel's row2uid
 * (nullable) by the fusion.  Optional ColBERT channel: colbert_ids / colbert_scores [nq, kc] are finished lists, written
 * by amdr_scope_maxsim_search_device (or anything else) EARLIER on the same stream; kc = 0: none.
 * When both tables' rows_max fit one slab of their channel (dense 256 rows, BM25 1 024, or the AMDR_SCOPE_SLAB pin) and
 * kd + kb + kc <= 32 this is ONE launch (scope_hybrid_kernel: one block per query from its first row to its fused hits;
 * no workspace, no reserve needed, no state in any handle between launches; AMDR_SCOPE_OVERLAP=0 pins its sequential
 * phase order, same results).  Every other shape, and AMDR_SCOPE_FUSED=0,
 * runs the three calls named above inside: they need the reserve and return AMDR_EINVAL beyond it.  Either way the call
 * only enqueues on `stream` and allocates nothing (capturable).  All three handles on one device (AMDR_EINVAL). */
int amdr_hybrid_scope_device(amdr_scope_t* h, amdr_dense_t* dense, amdr_bm25_t* bm25, const float* Q_dev,
                             const int32_t* q_terms_dev, const int64_t* q_ptr_dev, const int64_t* d_scope_ptr_dev,
                             const int64_t* d_rows_dev, const int32_t* d_qscope_dev, int32_t d_n_scopes, int64_t d_rows_max,
                             const int64_t* b_scope_ptr_dev, const int64_t* b_rows_dev, const int32_t* b_qscope_dev,
                             int32_t b_n_scopes, int64_t b_rows_max, int32_t nq, int32_t kd, int32_t kb,
                             const amdr_fuse_params_t* params, const int64_t* dense_row2uid, const int64_t* bm25_row2uid,
                             const int64_t* colbert_ids, const float* colbert_scores, int32_t kc,
                             const int64_t* colbert_row2uid, float* dense_scores, int64_t* dense_ids, double* bm25_scores,
                             int64_t* bm25_ids, int64_t* out_ids, double* out_vals, int32_t* out_mask, int32_t* out_count,
                             void* stream);
/* Host-only (no device is touched): *fused = 1 when amdr_hybrid_scope_device of these sizes takes the one-launch form
 * (AMDR_SCOPE_FUSED and AMDR_SCOPE_SLAB are read per call), *lds_bytes = the dynamic LDS of that launch (0 otherwise). */
int amdr_hybrid_scope_plan(int32_t nq, int32_t kd, int32_t kb, int32_t kc, int64_t rows_max_dense, int64_t rows_max_bm25,
                           int32_t* fused, int64_t* lds_bytes);
int amdr_scope_dense_search(amdr_scope_t* h, amdr_dense_t* dense, const float* Q_host, const int64_t* scope_ptr,
                            const int64_t* rows, const int32_t* qscope, int32_t n_scopes, int32_t nq, int32_t k,
                            float* scores_host, int64_t* ids_host);
int amdr_scope_bm25_search(amdr_scope_t* h, amdr_bm25_t* bm25, const int32_t* q_terms, const int64_t* q_ptr,
                           const int64_t* scope_ptr, const int64_t* rows, const int32_t* qscope, int32_t n_scopes,
                           int32_t nq, int32_t k, double* scores_host, int64_t* ids_host);
int amdr_scope_maxsim_search(amdr_scope_t* h, amdr_maxsim_t* maxsim, const float* Q_host, int32_t q_len,
                             const int64_t* scope_ptr, const int64_t* rows, const int32_t* qscope, int32_t n_scopes,
                             int32_t nq, int32_t k, float* scores_host, int64_t* ids_host);
int amdr_scope_destroy(amdr_scope_t* h);

/* ---- required and excluded terms: Boolean term constraints resolved into a scope table on the device ---------------
 * No reference counterpart: the reference's BM25 channel only prefers a query's terms (legalrag/retrieval/
 * bm25_retriever.py:74-75) and HybridRetriever.search has no filter argument; a caller who wants "articles that contain
 * seller and goods but not buyer" over-fetches and filters on the host.  csrc/term_scope.hip, csrc/term_scope_rule.hpp.
 * A constraint is a list of groups; a group is a non-empty list of term ids with a kind: 0 MUST, 1 ANY, 2 NOT.  The id -1
 * (any id outside [0, n_terms)) is a token the vocabulary does not hold: present in no document.  A document satisfies a
 * group when it has a posting for EVERY term of the group — a conjunction: the words anywhere, in any order.  The words
 * in sequence are a phrase: amdr_phrase_lists below resolves it into a virtual posting list, which
 * amdr_term_scope_lists takes as one more term.  It qualifies when it satisfies every MUST group, at least one ANY group (or there is none), no NOT group,
 * and lies in the constraint's base scope, if it has one.
 * Operands: grp_ptr i64 [n_cons + 1] indexes the groups of each constraint, grp_kind i32 [n_groups], grp_term_ptr i64
 * [n_groups + 1] indexes grp_terms i32; base_ptr i64 [n_base + 1] indexes base_rows i64 (each base scope strictly
 * ascending rows of [0, n_docs), as a scope table holds them), cons_base i32 [n_cons] names each constraint's base scope,
 * -1: the whole corpus.
 * Output: a scope table in the format of the scoped searches above — out_scope_ptr i64 [n_cons + 1], out_rows i64
 * [rows_cap], each constraint's qualifying documents strictly ascending — to be handed unchanged, with rows_max =
 * cand_max, to amdr_scope_*_search_device / amdr_hybrid_scope_device on the same stream (BM25 documents; the dense and
 * the ColBERT channel take it where they share the BM25 index's chunk list).  Scores do not change: idf and avgdl stay
 * those of the whole index.  out_status i32 [n_cons]: 0; 1 = the constraint's driver is longer than cand_max, its scope
 * is left empty; 2 = rows of the constraint lay at positions >= rows_cap and were dropped (scope_ptr is clamped to
 * rows_cap).  The other constraints of the call are exact either way.
 * The driver of a constraint — its candidates — is the shortest of { its base scope, the posting list of each term of
 * its MUST groups }, ties -> the first in that order; an unknown term among the MUST terms makes it empty without
 * reading anything; with no MUST term and no base scope the candidates are the documents 0 .. n_docs-1 themselves and the
 * work is proportional to the corpus.  Otherwise work is |driver| x the sum of log2(df) of the other terms: proportional
 * to the constraint.  cand_max >= the longest driver and rows_cap >= the sum of the drivers always suffice.
 * Three launches (count, scan, write; grid = constraints x tiles of 1 024 candidates), no atomics, deterministic.
 * amdr_term_scope_plan is host-only arithmetic: the workspace bytes of a call (16 B + 1 KiB per constraint and tile).
 * amdr_term_scope_device only enqueues on `stream` and allocates nothing (capturable); AMDR_EINVAL, enqueueing nothing,
 * for a null handle or array, a negative size, cand_max beyond 65 535 tiles, or work_bytes below the plan.  The handle
 * itself has no notion of a row shard: a deployment whose BM25 handle holds one rank's rows refuses a term constraint
 * above this call (retrieval/engine.py), since the base rows and the table would be global.  It does not validate the
 * operands' contents: terms outside the vocabulary and base rows outside [0, n_docs) are never dereferenced.
 * amdr_term_scope is the host-pointer twin: it validates (AMDR_EINVAL: a pointer array that does not start at 0 or is not
 * monotone, grp_ptr not ending at n_groups, an empty group, a kind outside 0 .. 2, base rows not strictly ascending or
 * outside [0, n_docs), cons_base outside [-1, n_base)), stages the operands, runs on the BM25 handle's own stream under
 * its mutex and returns the table (out_rows holds rows_cap values; the first out_scope_ptr[n_cons] are written) and the
 * status array in the host buffers. */
int amdr_term_scope_plan(int64_t n_cons, int64_t cand_max, int64_t* work_bytes);
int amdr_term_scope_device(amdr_bm25_t* bm25, const int64_t* grp_ptr_dev, const int32_t* grp_kind_dev,
                           const int64_t* grp_term_ptr_dev, const int32_t* grp_terms_dev, const int64_t* base_ptr_dev,
                           const int64_t* base_rows_dev, const int32_t* cons_base_dev, int64_t n_base, int64_t n_cons,
                           int64_t n_groups, int64_t cand_max, int64_t rows_cap, int64_t* out_scope_ptr_dev,
                           int64_t* out_rows_dev, int32_t* out_status_dev, void* work_dev, int64_t work_bytes, void* stream);
int amdr_term_scope(amdr_bm25_t* bm25, const int64_t* grp_ptr, const int32_t* grp_kind, const int64_t* grp_term_ptr,
                    const int32_t* grp_terms, const int64_t* base_ptr, const int64_t* base_rows, const int32_t* cons_base,
                    int64_t n_base, int64_t n_cons, int64_t n_groups, int64_t cand_max, int64_t rows_cap,
                    int64_t* out_scope_ptr, int64_t* out_rows, int32_t* out_status);

/* ---- phrase constraints: exact token sequences resolved into virtual posting lists on the device -------------------
 * No reference counterpart (the reference scores bags of words and keeps no token order).  csrc/phrase_scope.hip,
 * csrc/phrase_rule.hpp.  Needs the token stream of amdr_bm25_set_tokens.
 * A phrase is a list of L term ids, 2 <= L <= 16.  A document d HOLDS it when tokens[p + j] == phrase[j] for all j, for
 * some p with doc_ptr[d] <= p <= doc_ptr[d + 1] - L: a match never reaches into the next document; overlapping occurrences
 * and repeated tokens are plain cases of this.  An id outside [0, n_terms) anywhere in the phrase gives an empty list
 * without reading anything.
 * Operands: phr_ptr i64 [n_phr + 1] indexes phr_terms i32.  Output: out_list_ptr i64 [n_phr + 1] indexes out_docs i32
 * [rows_cap], each phrase's documents strictly ascending — a posting list in the resident format.  out_status i32 [n_phr]
 * holds the words of amdr_term_scope: 0; 1 = the phrase's driver is longer than cand_max, its list is left empty; 2 =
 * documents of the phrase lay at positions >= rows_cap and were dropped (list_ptr is clamped to rows_cap).
 * The driver of a phrase is the shortest posting list among its tokens, ties -> the first in phrase order, so the output
 * is ascending without a sort; work is |driver| x the sum of log2(df) of the other tokens plus the lengths of the
 * documents that hold all the tokens — not the corpus.  cand_max >= the smallest document frequency among a phrase's
 * tokens, maximised over the phrases, and rows_cap >= the sum of these always suffice.
 * Three launches (count, scan, write; grid = phrases x tiles of 256 candidates), no atomics, deterministic.
 * amdr_phrase_lists_plan is host-only arithmetic: the workspace bytes of a call (16 B + 1 KiB per phrase and tile).
 * amdr_phrase_lists_device only enqueues on `stream` and allocates nothing (capturable); AMDR_EINVAL, enqueueing nothing,
 * for a null handle, no resident stream, a null operand, a negative size, cand_max beyond 65 535 tiles, or work_bytes
 * below the plan.  It does not validate the operands' contents: a phrase whose length is outside 2 .. 16 gets an empty
 * list.  amdr_phrase_lists is the host-pointer twin: it validates (AMDR_EINVAL: phr_ptr not starting at 0 or not
 * monotone, a length outside 2 .. 16), stages, runs on the BM25 handle's own stream under its mutex and returns the
 * lists (the first out_list_ptr[n_phr] values of out_docs are written) and the status array in the host buffers.
 *
 * amdr_term_scope_lists* are amdr_term_scope* with three more operands, the virtual lists of the call: x_ptr i64
 * [n_x + 1] indexes x_doc i32, and the term id n_terms + p, p < n_x, names the list x_doc[x_ptr[p] .. x_ptr[p + 1]) —
 * in a MUST, ANY or NOT group, beside plain terms inside a group, and as the driver of a constraint.  Handed the outputs
 * of amdr_phrase_lists_device on the same stream, a phrase works wherever a token works; the rule of amdr_term_scope is
 * untouched and n_x = 0 is that call itself.  Status, plan and workspace are unchanged.  The host twin also validates
 * the lists (AMDR_EINVAL: x_ptr not starting at 0 or not monotone, a document outside [0, n_docs) or a list not strictly
 * ascending).
 * The bound.  A host that packs constraints knows only an UPPER bound for a virtual list's length: the smallest
 * document frequency among the phrase's tokens.  The device's driver is the shortest of the TRUE lengths, each <= its
 * upper bound; so cand_max = the longest driver and rows_cap = the sum of the drivers, computed by the rule above with the
 * upper bounds in place of the lengths, always suffice (tests/test_phrase_scope_gpu.py). */
int amdr_phrase_lists_plan(int64_t n_phr, int64_t cand_max, int64_t* work_bytes);
int amdr_phrase_lists_device(amdr_bm25_t* bm25, const int64_t* phr_ptr_dev, const int32_t* phr_terms_dev, int64_t n_phr,
                             int64_t cand_max, int64_t rows_cap, int64_t* out_list_ptr_dev, int32_t* out_docs_dev,
                             int32_t* out_status_dev, void* work_dev, int64_t work_bytes, void* stream);
int amdr_phrase_lists(amdr_bm25_t* bm25, const int64_t* phr_ptr, const int32_t* phr_terms, int64_t n_phr, int64_t cand_max,
                      int64_t rows_cap, int64_t* out_list_ptr, int32_t* out_docs, int32_t* out_status);
int amdr_term_scope_lists_device(amdr_bm25_t* bm25, const int64_t* grp_ptr_dev, const int32_t* grp_kind_dev,
                                 const int64_t* grp_term_ptr_dev, const int32_t* grp_terms_dev, const int64_t* base_ptr_dev,
                                 const int64_t* base_rows_dev, const int32_t* cons_base_dev, const int64_t* x_ptr_dev,
                                 const int32_t* x_doc_dev, int64_t n_x, int64_t n_base, int64_t n_cons, int64_t n_groups,
                                 int64_t cand_max, int64_t rows_cap, int64_t* out_scope_ptr_dev, int64_t* out_rows_dev,
                                 int32_t* out_status_dev, void* work_dev, int64_t work_bytes, void* stream);
int amdr_term_scope_lists(amdr_bm25_t* bm25, const int64_t* grp_ptr, const int32_t* grp_kind, const int64_t* grp_term_ptr,
                          const int32_t* grp_terms, const int64_t* base_ptr, const int64_t* base_rows,
                          const int32_t* cons_base, const int64_t* x_ptr, const int32_t* x_doc, int64_t n_x, int64_t n_base,
                          int64_t n_cons, int64_t n_groups, int64_t cand_max, int64_t rows_cap, int64_t* out_scope_ptr,
                          int64_t* out_rows, int32_t* out_status);

/* ---- proximity constraints: Near(t0, t1, ..., distance = n), beside phrases in one list array ------------------------
 * No reference counterpart (the reference scores bags of words and keeps no token order).  csrc/phrase_scope.hip,
 * csrc/near_rule.hpp.  Needs the token stream of amdr_bm25_set_tokens.
 * amdr_span_lists* are amdr_phrase_lists* over ITEMS of three kinds, so that the phrases and the Nears of one batch land
 * in ONE list array (amdr_term_scope_lists takes a single x_ptr / x_doc).  item_ptr i64 [n_items + 1] indexes item_terms
 * i32; item_kind i32 [n_items]: 0 a phrase (the rule above; item_dist is not read), 1 a Near unordered, 2 a Near ordered;
 * item_dist i32 [n_items]: a Near's distance n.
 * A Near is M term ids t[0 .. M), 2 <= M <= 8 — repeats are allowed and are meaningful — and a distance 1 <= n <= 255.
 *   unordered  a document HOLDS it when some run of at most n + 1 consecutive tokens of it contains every distinct term
 *              at least as many times as the Near names it (two different tokens at p and q: |q - p| <= n);
 *   ordered    a document HOLDS it when there are positions p0 < p1 < ... < p[M-1] inside it with tokens[p_i] == t[i]
 *              and p[M-1] - p0 <= n.
 * A window never reaches into the next document; at a document's end it is clamped.  Near(a, b, 1, ordered) is the
 * phrase (a, b); with n >= the longest document the unordered form is the conjunction with multiplicities.  An id
 * outside [0, n_terms) anywhere in a Near gives an empty list without reading anything.
 * Outputs, status words, driver (the shortest posting list among the tokens, ties -> the first), bounds, launches and
 * workspace are those of amdr_phrase_lists: amdr_span_lists_plan is the phrase plan's arithmetic, and a call whose items
 * are all of kind 0 writes the bytes amdr_phrase_lists writes.  One wave walks one surviving document, 64 anchor
 * positions per round, from a staged run of at most 64 + n tokens; worst case len x (n + 1) steps per document.
 * amdr_span_lists_device only enqueues and allocates nothing (capturable); it refuses what amdr_phrase_lists_device
 * refuses, and does not validate the operands' contents: an item with a kind outside 0 .. 2, a length outside its
 * kind's range or a Near distance outside 1 .. 255 gets an empty list.  amdr_span_lists is the host-pointer twin: it
 * validates (AMDR_EINVAL: item_ptr not starting at 0 or not monotone, a kind outside 0 .. 2, a phrase length outside
 * 2 .. 16, a Near length outside 2 .. 8, a distance outside 1 .. 255), stages, runs on the BM25 handle's own stream under
 * its mutex and returns the lists and the status array in the host buffers. */
int amdr_span_lists_plan(int64_t n_items, int64_t cand_max, int64_t* work_bytes);
int amdr_span_lists_device(amdr_bm25_t* bm25, const int64_t* item_ptr_dev, const int32_t* item_terms_dev,
                           const int32_t* item_kind_dev, const int32_t* item_dist_dev, int64_t n_items, int64_t cand_max,
                           int64_t rows_cap, int64_t* out_list_ptr_dev, int32_t* out_docs_dev, int32_t* out_status_dev,
                           void* work_dev, int64_t work_bytes, void* stream);
int amdr_span_lists(amdr_bm25_t* bm25, const int64_t* item_ptr, const int32_t* item_terms, const int32_t* item_kind,
                    const int32_t* item_dist, int64_t n_items, int64_t cand_max, int64_t rows_cap, int64_t* out_list_ptr,
                    int32_t* out_docs, int32_t* out_status);

/* ---- unions of posting lists: the root expander (sell!) and alternatives (buyer OR purchaser) -------------------------
 * No reference counterpart (the reference has no stemmer and no filter; every token is compared exactly).
 * csrc/union_lists.hip, csrc/union_rule.hpp.  Needs the postings only: a handle WITHOUT a token stream resolves unions.
 * A union item is M >= 0 term ids, item_terms[item_ptr[p] .. item_ptr[p + 1]).  Its list is the strictly ascending set
 * of the documents that have a posting for at least one of them.  An id outside [0, n_terms) names a token present in no
 * document and contributes nothing (never dereferenced); M = 0, or every id unknown, gives an empty list; a repeated id is
 * harmless.  The lists are merged and de-duplicated, not concatenated: a document two terms share stands once.
 * One list array.  amdr_term_scope_lists takes a single x_ptr / x_doc, so the call CONTINUES the array a span step began:
 * list_ptr_dev holds n_before + n_items + 1 entries, of which the first n_before + 1 were written earlier on the same
 * stream; start = list_ptr[n_before] is read on the device (no host synchronise), the entries n_before + 1 .. are
 * written and the items' documents are appended behind `start`.  rows_cap is the capacity of the WHOLE docs array.
 * n_before = 0 starts an array: the call writes list_ptr[0] = 0 itself.
 *   out_status i32 [n_items]   0, or 2 (the meaning of amdr_term_scope's: documents of the item lie at positions >=
 *                              rows_cap and were dropped; list_ptr is clamped to rows_cap).  There is no 1: a union has
 *                              no driver.  Bound a host packer knows: min(n_docs, the sum of the document frequencies of
 *                              the item's distinct known ids) >= the list's length; rows_cap = the sum of these (plus what
 *                              stands before) always suffices.
 * Three launches (count, scan, write), no global atomics, deterministic, nothing allocated, capturable.  The grid is
 * one-dimensional: n_items x tiles cells, tiles = max(1, ceil(n_docs / 32 768)); a cell is a 4 KiB bitmap of its tile's
 * documents, set in LDS and parked in the workspace between the passes.  Work per cell: M x 2 binary searches plus the
 * postings inside the tile — an item of 4 096 terms on 10 M documents is 306 tiles x 4 096 x 2 searches.
 * amdr_union_lists_plan is host-only arithmetic: the workspace of n_items items on an index of n_docs documents (two i64
 * and 4 KiB per cell).  amdr_union_lists_device only enqueues; it does not validate the operands' contents and returns
 * AMDR_EINVAL, enqueueing nothing and leaving the outputs untouched, for a null handle or array, a negative size, more
 * cells than one launch takes (n_items x tiles x 256 threads must stay below 2^32, so n_items x tiles >= 2^31 is always
 * refused) or work_bytes below the plan.  amdr_union_lists is the host-pointer twin: it starts its own array
 * (n_before = 0), validates (AMDR_EINVAL: item_ptr not starting at 0 or not monotone), stages, runs on the BM25 handle's
 * own stream under its mutex and returns the lists and the status array in the host buffers.
 * Mutations: amdr_bm25_add's rule; n_docs changes the tile count, so callers plan and capture again. */
int amdr_union_lists_plan(int64_t n_items, int64_t n_docs, int64_t* work_bytes);
int amdr_union_lists_device(amdr_bm25_t* bm25, const int64_t* item_ptr_dev, const int32_t* item_terms_dev, int64_t n_items,
                            int64_t n_before, int64_t rows_cap, int64_t* list_ptr_dev, int32_t* docs_dev,
                            int32_t* out_status_dev, void* work_dev, int64_t work_bytes, void* stream);
int amdr_union_lists(amdr_bm25_t* bm25, const int64_t* item_ptr, const int32_t* item_terms, int64_t n_items, int64_t rows_cap,
                     int64_t* out_list_ptr, int32_t* out_docs, int32_t* out_status);

/* ---- class spans: a root expander or alternatives INSIDE a phrase or a Near (sell! /5 good!, "secur! interest") -------
 * No reference counterpart (the reference keeps no token order and has no stemmer).  csrc/class_span.hip,
 * csrc/class_span_rule.hpp.  Needs the token stream (amdr_bm25_set_tokens) and the list array of the call.
 * An item is L slot ids item_slots[item_ptr[p] .. item_ptr[p + 1]), a kind (0 phrase: 2 <= L <= 16; 1 Near unordered, 2
 * Near ordered: 2 <= L <= 8, 1 <= item_dist[p] <= 255) — the kinds and sizes of amdr_span_lists.  A slot id s is
 *   0 <= s < n_terms                                        a plain token;
 *   n_terms + cls_first <= s < n_terms + cls_first + n_cls  class c = s - n_terms - cls_first: its member ids are
 *                                                           cls_terms[cls_ptr[c] .. cls_ptr[c + 1]), strictly ascending
 *                                                           (the item_ptr / item_terms of the union step), and its document
 *                                                           list is list cls_first + c of the list array, written earlier
 *                                                           on the same stream by amdr_union_lists_device;
 *   anything else                                           unknown: the item's list is empty, nothing is dereferenced.
 * A token FILLS a slot when it equals the plain token or is a member of the class.  A document holds a phrase item when
 * some position p has token p + j filling slot j for every j; an ordered Near when positions p0 < p1 < ... carry tokens
 * that fill the slots in order, the last at most dist behind the first; an unordered Near when some run of at most
 * dist + 1 consecutive tokens admits an assignment of the slots to distinct positions of the run.  Never across two
 * documents.  The unordered form is resolved with the first-unfilled-slot tally, which equals that matching when the
 * slots' id sets are pairwise EQUAL OR DISJOINT; the host twin refuses an unordered item that breaks this.
 * One list array, continued as amdr_union_lists_device continues it: list_ptr_dev holds n_before + n_items + 1 entries of
 * which the first n_before + 1 were written earlier on the same stream, cls_first + n_cls <= n_before; start =
 * list_ptr[n_before] is read on the device, the entries n_before + 1 .. are written and the items' documents are appended
 * behind `start`.  rows_cap is the capacity of the WHOLE docs array.  n_before = 0 starts an array.
 *   out_status i32 [n_items]   0; 1: the item's driver — the shortest of its slots' lists, found on the device — is longer
 *                              than cand_max, the list is left empty; 2: documents at positions >= rows_cap were dropped,
 *                              list_ptr is clamped.  An undefined item or an unknown slot: an empty list, status 0.  Bound a
 *                              host packer knows: the smallest slot bound (df of a plain id, min(n_docs, sum of df) of a
 *                              class) >= the driver >= the list.
 * Three launches (count, scan, write), no global atomics, deterministic, nothing allocated, capturable.  The grid is
 * one-dimensional: n_items x tiles cells, tiles = max(1, ceil(cand_max / 256)).  Each token of a surviving document is
 * turned once per round into the mask of the slots it fills; worst case one round of 319 tokens x 16 class slots x 12
 * dependent loads (a class of 4 096 ids).
 * amdr_class_spans_plan is host-only arithmetic (two i64 and 1 KiB per cell).  amdr_class_spans_device only enqueues; it
 * does not validate the operands' contents and returns AMDR_EINVAL, enqueueing nothing and leaving the outputs untouched,
 * for a null handle or array, a negative size, classes that do not lie among the n_before lists, n_items x tiles x 256 >=
 * 2^32, work_bytes below the plan or a handle without a token stream.  amdr_class_spans is the host-pointer twin: class c is
 * the slot id n_terms + c; it validates (AMDR_EINVAL: item_ptr or cls_ptr not monotone from 0, a kind, length or distance
 * out of range, member ids not strictly ascending, overlapping unequal slots in an unordered item), runs the union step
 * for the classes and then this step in an array of its own on the BM25 handle's stream under its mutex, and returns only
 * the items' lists, rebased to 0, with rows_cap applied to them alone.
 * Mutations: amdr_bm25_add's rule; an update drops the token stream. */
int amdr_class_spans_plan(int64_t n_items, int64_t cand_max, int64_t* work_bytes);
int amdr_class_spans_device(amdr_bm25_t* bm25, const int64_t* item_ptr_dev, const int32_t* item_slots_dev,
                            const int32_t* item_kind_dev, const int32_t* item_dist_dev, int64_t n_items,
                            const int64_t* cls_ptr_dev, const int32_t* cls_terms_dev, int64_t n_cls, int64_t cls_first,
                            int64_t n_before, int64_t cand_max, int64_t rows_cap, int64_t* list_ptr_dev, int32_t* docs_dev,
                            int32_t* out_status_dev, void* work_dev, int64_t work_bytes, void* stream);
int amdr_class_spans(amdr_bm25_t* bm25, const int64_t* item_ptr, const int32_t* item_slots, const int32_t* item_kind,
                     const int32_t* item_dist, int64_t n_items, const int64_t* cls_ptr, const int32_t* cls_terms, int64_t n_cls,
                     int64_t cand_max, int64_t rows_cap, int64_t* out_list_ptr, int32_t* out_docs, int32_t* out_status);

/* ---- unit spans: same sentence, same paragraph (csrc/unit_span.hip, csrc/unit_span_rule.hpp) --------
 * No reference counterpart.  buyer /s seller: "one provision speaks of both".
 * The break flags lie beside the token stream of amdr_bm25_set_tokens, one byte per token: bit 0 (value 1) the token begins a
 * sentence, bit 1 (value 2) it begins a paragraph; a paragraph start is a sentence start, so a byte is 0, 1 or 3.  The first
 * token of a document begins both, whatever its byte says.  The flagged tokens partition a document into units.
 * amdr_bm25_set_breaks needs a resident stream of exactly n_tokens tokens and refuses (AMDR_EINVAL, the handle keeps what it
 * had) any other count and any byte outside {0, 1, 3}.  The flags describe ONE state of the stream: amdr_bm25_set_tokens,
 * every successful update — plain or carrying; the carry kernels do not carry the flags — and whatever else drops the stream
 * drop them.  amdr_bm25_breaks_info: out2[0] 1 if flags are resident else 0, out2[1] their count.  amdr_bm25_read_breaks
 * copies them back (AMDR_EINVAL without flags).
 * A unit item is L slot ids, 2 <= L <= 8, exactly as a class span's (a plain term id, or n_terms + cls_first + c for class c),
 * and a kind: bit 0 ordered, bit 1 paragraph (else sentence).  Within one document
 *   unordered  some unit admits an assignment of the slots to DISTINCT positions of the unit, each token filling its slot (a
 *              bipartite matching; slots with different ids must name disjoint token sets — equal sets share one id);
 *   ordered    positions p0 < p1 < ... inside one unit, token p_i filling slot i.
 * An item the rule does not define (a length or kind out of range, an unknown slot) gets an empty list; nothing is
 * dereferenced for it.  Item p's list is the ascending documents that hold it, appended to the call's list array behind the
 * n_before lists already there (the class spans' last), status as amdr_term_scope: 1 the driver — the shortest slot list —
 * exceeds cand_max, 2 rows dropped at rows_cap.  Three launches (count, scan, write), no global atomics, deterministic,
 * nothing allocated or cleared, capturable; grid n_items x max(1, ceil(cand_max / 256)) cells.  The count pass walks a
 * surviving document 64 tokens per round — 4 B of token and 1 B of flag per lane, each read once — and decides every round
 * from the wave's ballots.
 * amdr_unit_spans_plan is host-only arithmetic (two i64 and 1 KiB per cell).  amdr_unit_spans_device only enqueues; it does
 * not validate the operands' contents and returns AMDR_EINVAL, enqueueing nothing, for a null handle or array, a negative
 * size, classes that do not lie among the n_before lists, too many cells, work_bytes below the plan, or a handle without a
 * token stream or without break flags.  amdr_unit_spans is the host-pointer twin: class c is the slot id n_terms + c; it
 * validates (AMDR_EINVAL), runs the union step for the classes and then this step in an array of its own on the BM25
 * handle's stream under its mutex, and returns only the items' lists, rebased to 0. */
int amdr_bm25_set_breaks(amdr_bm25_t* h, const uint8_t* brk, int64_t n_tokens);
int amdr_bm25_breaks_info(amdr_bm25_t* h, int64_t* out2);
int amdr_bm25_read_breaks(amdr_bm25_t* h, uint8_t* out);
int amdr_unit_spans_plan(int64_t n_items, int64_t cand_max, int64_t* work_bytes);
int amdr_unit_spans_device(amdr_bm25_t* bm25, const int64_t* item_ptr_dev, const int32_t* item_slots_dev,
                           const int32_t* item_kind_dev, int64_t n_items, const int64_t* cls_ptr_dev, const int32_t* cls_terms_dev,
                           int64_t n_cls, int64_t cls_first, int64_t n_before, int64_t cand_max, int64_t rows_cap,
                           int64_t* list_ptr_dev, int32_t* docs_dev, int32_t* out_status_dev, void* work_dev, int64_t work_bytes,
                           void* stream);
int amdr_unit_spans(amdr_bm25_t* bm25, const int64_t* item_ptr, const int32_t* item_slots, const int32_t* item_kind,
                    int64_t n_items, const int64_t* cls_ptr, const int32_t* cls_terms, int64_t n_cls, int64_t cand_max,
                    int64_t rows_cap, int64_t* out_list_ptr, int32_t* out_docs, int32_t* out_status);

/* ---- marks and best passages of the hit documents (csrc/marks.hip, csrc/marks_rule.hpp) --------
 * No reference counterpart.  For every (query, hit) pair: which tokens of the hit document the query MARKS, and the window
 * of `window` tokens that holds the most of the query — term highlighting and the best-passage snippet, from the resident
 * token stream (amdr_bm25_set_tokens; the carrying updates keep it).
 *   docs i64 [nq, ld_docs]          the hit ids, k per query (ld_docs >= k); -1: no hit.
 *   mk_ptr i64 [nq + 1], mk_terms i32, mk_slot i32   query q's mark table: mk_terms[mk_ptr[q] .. mk_ptr[q + 1]) strictly
 *                                   ascending, distinct term ids; mk_slot, parallel, the SLOT 0 .. 31 the token fills.  A slot
 *                                   is one query word: a plain token or a class (a Prefix's tokens, a OneOf's members).  A
 *                                   token outside the table fills nothing.
 *   slot_w f64 [nq, 32]             the slots' weights.
 *   slot_loose u32 [nq]             bit s: slot s marks its token wherever it stands.
 *   sq_ptr i64 [nq + 1], sq_off i64 [n_seq + 1], sq_slots i32   query q's sequences sq_ptr[q] .. sq_ptr[q + 1]; sequence s is
 *                                   the L slots sq_slots[sq_off[s] .. sq_off[s + 1]), 2 <= L <= 16: a phrase.  It OCCURS at
 *                                   position p of a document when token p + j fills slot j of it for every j and p + L stays
 *                                   inside the document.
 * Position p is MARKED when m(p) = (slot mask of token p & slot_loose[q]) | cover(p) != 0, cover(p) the OR of the slot of
 * member j over every occurrence at p - j; its slot is the lowest set bit of m(p).  A slot that is only a phrase member
 * marks a token only inside an occurrence of the phrase.  The candidates of the best window are [a, a + window) for every
 * marked a, clamped to the document; the score is the sum of slot_w over the DISTINCT slots of the window's marks, added
 * in ascending slot order in fp64; the greatest score wins, ties -> the smallest a.  Marks are kept in position order up to
 * 1 024 per document; later ones are counted only, and the best window is the best among the kept anchors (status 1).
 *   out_win i32 [nq, k, 4]          window start (relative to the document), window end (exclusive), marks in the window,
 *                                   marks in the document (the true count).  No mark: [0, min(window, len)), 0, 0.
 *   out_score f64 [nq, k]           the window's score; 0.0 without marks.
 *   out_slots u32 [nq, k, 2]        the slots in the window, the slots among the kept marks.
 *   out_marks i32 [nq, k, marks_cap, 2]   the first marks_cap marks of the window as (relative position, slot), ascending;
 *                                   the rest (-1, -1).  May be null when marks_cap is 0.
 *   out_status i32 [nq, k]          0; 1: more than 1 024 marks.
 * A hit id of -1 — in the "_device" form any id outside [0, n_docs) — gives zeros, fill marks and status 0 and reads
 * nothing.  Outputs are packed [nq, k] whatever ld_docs is.
 * One launch, one wave per pair in the grid's x, LDS only (6 016 B per wave whatever the document's length): no workspace,
 * no global atomics, deterministic.  Work: the tokens of the hit documents x log2 of the mark table, plus kept marks x
 * marks per window.
 * amdr_bm25_marks_device only enqueues and allocates nothing (capturable).  It does not validate the operands' contents —
 * a sequence with a slot outside 0 .. 31 or a length outside 2 .. 16 never occurs, a table slot outside 0 .. 31 fills
 * nothing, and no value of docs_dev makes it read out of bounds — and returns AMDR_EINVAL, enqueueing nothing and leaving
 * the outputs untouched, for a null handle, operand or output, a handle without a token stream, a negative size, ld_docs
 * < k, nq x k >= 2^31, window outside 1 .. 4096 or marks_cap outside 0 .. 64.  amdr_bm25_marks is the host-pointer twin: it
 * validates (AMDR_EINVAL: pointers not monotone from 0, terms not strictly ascending or outside [0, n_terms), a slot outside
 * 0 .. 31, a sequence length outside 2 .. 16, a weight that is not finite, a hit id outside [-1, n_docs)), stages the
 * operands in device arrays that live for the call and runs on the handle's own stream under its mutex.
 * amdr_bm25_marks_kernel_ms: the device time of the kernel of the last amdr_bm25_marks; -1.0 when there is none.
 * Mutations: amdr_bm25_add's rule; a plain update drops the token stream, a carrying one keeps it. */
int amdr_bm25_marks_device(amdr_bm25_t* bm25, const int64_t* docs_dev, int64_t nq, int64_t k, int64_t ld_docs,
                           const int64_t* mk_ptr_dev, const int32_t* mk_terms_dev, const int32_t* mk_slot_dev,
                           const double* slot_w_dev, const uint32_t* slot_loose_dev, const int64_t* sq_ptr_dev,
                           const int64_t* sq_off_dev, const int32_t* sq_slots_dev, int32_t window, int32_t marks_cap,
                           int32_t* out_win_dev, double* out_score_dev, uint32_t* out_slots_dev, int32_t* out_marks_dev,
                           int32_t* out_status_dev, void* stream);
int amdr_bm25_marks(amdr_bm25_t* bm25, const int64_t* docs, int64_t nq, int64_t k, int64_t ld_docs, const int64_t* mk_ptr,
                    const int32_t* mk_terms, const int32_t* mk_slot, const double* slot_w, const uint32_t* slot_loose,
                    const int64_t* sq_ptr, const int64_t* sq_off, const int32_t* sq_slots, int32_t window, int32_t marks_cap,
                    int32_t* out_win, double* out_score, uint32_t* out_slots, int32_t* out_marks, int32_t* out_status);
int amdr_bm25_marks_kernel_ms(amdr_bm25_t* h, double* ms);

/* ---- facets: a constraint's qualifying rows counted by the values of chunk fields (csrc/facet.hip, csrc/facet_rule.hpp) ----
 * No reference counterpart (the reference returns hits and counts nothing).  "How many provisions match, and how do they
 * spread over the statute": the result set is the scope table amdr_term_scope*_device or an upload left on the device.
 *   scope_ptr i64 [n_cons + 1], rows i64   constraint p's rows are rows[scope_ptr[p] .. scope_ptr[p + 1]), strictly
 *                                   ascending inside [0, n_rows).
 *   rows_max                        an upper bound on the longest scope, as the scoped searches take it; rows of a scope
 *                                   beyond it are not read.
 *   codes i32 [n_fields, n_rows]    field-major code columns: a value in [0, n_codes[f]) names a value of field f, any other
 *                                   value (-1 the canonical one) says the row has none.
 *   n_codes i64 [n_fields]          a HOST array in both forms; 1 <= n_fields <= 8, 0 <= n_codes[f] < 2^31.
 *   top                             1 .. AMDR_FACET_MAX_TOP.
 * Per constraint p and field f, R = p's rows:
 *   out_total i64 [n_cons]                  |R|
 *   out_missing i64 [n_cons, n_fields]      the rows of R whose code is outside [0, n_codes[f])
 *   out_distinct i32 [n_cons, n_fields]     the codes with a count > 0
 *   out_code i32 [n_cons, n_fields, top], out_count i64, the same shape
 *                                           the first `top` codes with count > 0 by (count descending, code ascending);
 *                                           slots past `distinct` hold code -1 and count 0.
 * An empty scope gives total 0, distinct 0 and an all-padding list; n_cons = 0 enqueues nothing.
 * Work: three launches.  zero: the counters, int32 [n_cons][sum of (n_codes[f] + 1)].  count: grid (n_cons x tiles,
 * n_fields), tiles = max(1, ceil(min(rows_max, n_rows) / AMDR_FACET_TILE_ROWS)); a block reads its tile's rows once, gathers
 * their codes and bins them — a field of n_codes <= AMDR_FACET_LDS_BINS in LDS, its non-zero bins then added to the global
 * counters, a wider field straight in global memory.  select: one block per (constraint, field) sweeps the counters and keeps
 * the best `top` keys (count, ~code) with the wave selectors of csrc/topk.hpp.  Integer adds: deterministic.
 * amdr_facet_plan is host-only arithmetic: the bytes of the counters.  amdr_facet_counts_device only enqueues on `stream`,
 * on the calling thread's current device, and allocates nothing (capturable; the call zeroes its counters itself, so a
 * captured call may be replayed).  It does not validate the operands' contents — a row outside [0, n_rows) is never
 * dereferenced and counted nowhere, out_total included — and returns AMDR_EINVAL, enqueueing nothing and leaving the outputs
 * untouched, for a null array, a negative size, n_rows >= 2^31, n_fields, an n_codes or top out of range, more than 2^24 - 1
 * cells (n_cons x tiles, or n_cons x n_fields) or work_bytes below the plan.  A batch past 65 535 constraints is one launch:
 * the constraints stand in the grid's x.  amdr_facet_counts is the host-pointer twin: it validates (AMDR_EINVAL: scope_ptr
 * not monotone from 0, a scope longer than rows_max, rows not strictly ascending inside [0, n_rows)), stages the operands
 * in the scope handle's staging buffer, runs on its stream under its mutex and returns the outputs in the host buffers. */
#define AMDR_FACET_TILE_ROWS 2048
#define AMDR_FACET_LDS_BINS 4096
#define AMDR_FACET_MAX_TOP 64
int amdr_facet_plan(int64_t n_cons, int32_t n_fields, const int64_t* n_codes, int64_t* work_bytes);
int amdr_facet_counts_device(const int64_t* scope_ptr_dev, const int64_t* rows_dev, int64_t n_cons, int64_t rows_max,
                             const int32_t* codes_dev, int64_t n_rows, int32_t n_fields, const int64_t* n_codes, int32_t top,
                             int64_t* out_total_dev, int64_t* out_missing_dev, int32_t* out_distinct_dev,
                             int32_t* out_code_dev, int64_t* out_count_dev, void* work_dev, int64_t work_bytes, void* stream);
int amdr_facet_counts(amdr_scope_t* h, const int64_t* scope_ptr, const int64_t* rows, int64_t n_cons, int64_t rows_max,
                      const int32_t* codes, int64_t n_rows, int32_t n_fields, const int64_t* n_codes, int32_t top,
                      int64_t* out_total, int64_t* out_missing, int32_t* out_distinct, int32_t* out_code, int64_t* out_count);

/* ---- vocabulary patterns: Wildcard and Fuzzy resolved into term ids (csrc/vocab_match.hip, csrc/vocab_match_rule.hpp) ----
 * No reference counterpart: the reference looks a query token up exactly (legalrag/retrieval/bm25_retriever.py:74-75) and
 * has no pattern of any kind.  These calls stand beside retrieval/terms.py prefix_tokens, the host expansion of a Prefix: a
 * prefix is a contiguous range of the sorted vocabulary and is found by bisection; a wildcard or an edit-distance pattern
 * has no such range and replaces a Python loop over every token per pattern with one scan on the device.
 * amdr_vocab_t is a resident copy of the vocabulary as amdr_tokenizer_create takes it: a UTF-8 blob and offsets
 * i64 [n_terms + 1], term i the token with id i, plus the code-point count of every term, computed once at create.
 * amdr_vocab_create validates (AMDR_EINVAL: a null array, n_terms outside [0, 2^31), offsets that do not ascend from 0, a
 * term that is not well-formed UTF-8) and copies; the handle is small, separate from the tokeniser's and owns a stream and
 * a staging buffer for the host-pointer twin.  amdr_vocab_info: out2 = {n_terms, bytes of the blob}.
 *   pat_cp u32 [cp_total]            the patterns' code points back to back; in a Wildcard 0x110000 is '?' (exactly one
 *                                    code point) and 0x110001 is '*' (any run, the empty one included): two values above
 *                                    U+10FFFF, so a literal question mark in a TERM is an ordinary code point.
 *   pat_ptr i64 [n_pat + 1]          pattern p is pat_cp[pat_ptr[p] .. pat_ptr[p + 1]), 1 .. AMDR_VOCAB_MAX_PATTERN values.
 *   pat_kind i32 [n_pat], pat_arg    0 Wildcard (arg 0, at least one literal), 1 Fuzzy (arg = edits, 1 or 2: the
 *                                    optimal-string-alignment distance over code points, transpositions of two adjacent
 *                                    code points included, distance 0 included).
 *   item_cap                         1 .. AMDR_VOCAB_MAX_ITEMS: the stride of the outputs.
 *   ids i32 [n_pat, item_cap]        the first item_cap term ids pattern p names, ascending, then -1.
 *   dist u8 [n_pat, item_cap]        their distances (0 for a Wildcard), then 255.
 *   n_match i64 [n_pat]              the TRUE number of terms named, which may exceed item_cap.
 * The stride is fixed because nobody can bound a pattern's matches without running it: an over-wide pattern truncates its
 * own row and no neighbour's.  A term of zero bytes is named by nothing.
 * Work: three launches.  count: a one-dimensional grid of n_pat x tiles blocks, tiles = max(1, ceil(n_terms /
 * AMDR_VOCAB_TILE_TERMS)); a block stages its pattern in LDS, its threads stride over the tile's terms (length pre-test on
 * code-point counts, then the rule) and set bits of an LDS bitmap, which is counted and parked in the workspace.  scan:
 * the cells' offsets.  write: the parked bits expanded, ascending, into the pattern's row; the distance is computed again
 * for the kept terms only; the block of tile 0 writes n_match and pads the row.  No global atomics, nothing to clear.
 * amdr_vocab_match_plan is host-only arithmetic: per cell two i64 and the 1 KiB bitmap, each region aligned to 256 bytes.
 * amdr_vocab_match_device only enqueues on `stream`, on the calling thread's current device, and allocates nothing
 * (capturable; a captured call may be replayed over rewritten patterns).  It cannot validate the patterns' contents and is
 * safe for any: a span outside [0, cp_total) or of a length outside 1 .. 64, a kind or an argument out of range, a value
 * that is no code point (a reserved one in a Fuzzy included) or a Wildcard without a literal names nothing, n_match 0, and
 * nothing is read or written out of bounds.  It returns AMDR_EINVAL, enqueueing nothing and leaving the outputs untouched,
 * for a null handle or array, a negative size, item_cap out of range, more than 2^24 - 1 cells, work_bytes below the
 * plan or a workspace that is not aligned to 8 bytes (its int64 counts).  The current device must be the handle's: as in
 * the other "_device" calls, that is the caller's to see to.  A batch past 65 535 patterns is one launch.  amdr_vocab_match is the host-pointer twin: it validates the patterns
 * (AMDR_EINVAL: pat_ptr not monotone from 0 to cp_total, a length, kind, argument or value out of range, a Wildcard
 * without a literal), stages in the handle's buffer, runs on its stream under its mutex and returns the outputs. */
#define AMDR_VOCAB_TILE_TERMS 8192
#define AMDR_VOCAB_MAX_PATTERN 64
#define AMDR_VOCAB_MAX_ITEMS 4096
int amdr_vocab_create(const char* blob, const int64_t* offsets, int64_t n_terms, int32_t device, amdr_vocab_t** out);
int amdr_vocab_destroy(amdr_vocab_t* h);
int amdr_vocab_info(amdr_vocab_t* h, int64_t* out2);
int amdr_vocab_match_plan(int64_t n_terms, int64_t n_pat, int64_t* work_bytes);
int amdr_vocab_match_device(amdr_vocab_t* h, const uint32_t* pat_cp_dev, const int64_t* pat_ptr_dev, const int32_t* pat_kind_dev,
                            const int32_t* pat_arg_dev, int64_t n_pat, int64_t cp_total, int32_t item_cap, int32_t* ids_dev,
                            uint8_t* dist_dev, int64_t* n_match_dev, void* work_dev, int64_t work_bytes, void* stream);
int amdr_vocab_match(amdr_vocab_t* h, const uint32_t* pat_cp, const int64_t* pat_ptr, const int32_t* pat_kind,
                     const int32_t* pat_arg, int64_t n_pat, int64_t cp_total, int32_t item_cap, int32_t* out_ids,
                     uint8_t* out_dist, int64_t* out_n_match);

/* ---- multi-GPU: merge per-shard top-k after the RCCL all-gather --------
 * No reference counterpart (the reference is single-process).
 * parts: [n_parts, nq, k_in] scores + GLOBAL ids (-1 padding); output
 * [nq, k_out], score descending, ties -> lower global id. */
int amdr_merge_topk_f32_device(const float* scores, const int64_t* ids, int32_t n_parts, int32_t nq, int32_t k_in,
                               int32_t k_out, float* out_scores, int64_t* out_ids, int32_t device, void* stream);
int amdr_merge_topk_f64_device(const double* scores, const int64_t* ids, int32_t n_parts, int32_t nq, int32_t k_in,
                               int32_t k_out, double* out_scores, int64_t* out_ids, int32_t device, void* stream);

/* ---- multi-GPU: the shard exchange of ALL channels, one launch either side of the all-gather -------------------
 * No reference counterpart (single process; legalrag/config.py:106 `colbert_nranks = 1`).  SURVEY.md 8(b)/8(e):
 * rank r holds rows [offset_r, offset_r + n_r) of every channel; per query batch ONE all-gather of a packed int64
 * buffer carries every channel's per-shard top-k.
 *   row of query q (amdr_shard_row_words words) = for each channel c, in order:
 *       k_c score words (the score's bits as fp64; an fp32 score widens exactly) | k_c GLOBAL ids (-1 = padding)
 * amdr_shard_pack_device : this rank's lists (scores fp32 or fp64 [nq, k_c], LOCAL ids [nq, k_c]) -> send [nq, row];
 *                          global id = local id + id_offset.
 * amdr_shard_merge_device: gathered [world, nq, row] (the all-gather's output, read in place) -> per channel the global
 *                          top-k_c: out scores [nq, k_c] (fp32 / fp64 as flagged), out ids [nq, k_c]; score descending,
 *                          ties -> lower global id, -1 / -FLT_MAX (-DBL_MAX) padding.  Identical on every rank.
 * Ids and values: ANY negative id is "no entry" — the pack writes it to the wire unchanged (only ids >= 0 take the
 * offset), the merge skips it whatever its score word holds and pads its own output with -1 alone.  The id decides, never
 * the score: a valid hit may score -FLT_MAX / -DBL_MAX or -inf.  -0.0 ties with +0.0 (the lower id first) and comes back
 * as +0.0; a NaN ranks behind -inf and ahead of padding, and comes back as the NaN 0xfffffffe (fp32 channel) /
 * 0xfffffffffffffffe (fp64 channel) whatever payload went in — the bits amdr_merge_topk_*_device returns too.  Every
 * other hit returns the bits that went in.  id_offset >= 0; global ids use all 63 bits.
 * Both only enqueue on `stream` (graph-capturable); up to 4 channels, k_c <= AMDR_MAX_K. */
typedef struct amdr_shard_chan {
  void* scores;   /* pack: const input lists; merge: output */
  int64_t* ids;
  int32_t k;
  int32_t f64;    /* 1: scores are double (BM25), 0: float (dense, MaxSim) */
} amdr_shard_chan_t;
int amdr_shard_row_words(const amdr_shard_chan_t* chans, int32_t n_chan, int64_t* words);
int amdr_shard_pack_device(const amdr_shard_chan_t* chans, int32_t n_chan, int32_t nq, int64_t id_offset, int64_t* send,
                           int32_t device, void* stream);
int amdr_shard_merge_device(const int64_t* gathered, int32_t world, int32_t nq, const amdr_shard_chan_t* out_chans,
                            int32_t n_chan, int32_t device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMDRETRIEVAL_H */
