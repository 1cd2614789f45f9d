/*
 * mi355rec.h -- C ABI of libmi355rec.so, the MI355X (gfx950) implementation of the baseline training
 * kernels of MaurizioFD/RecSys2019_DeepLearning_Evaluation.
 *
 * The reference has no C/FFI boundary on this path: its "operator API" is the Python-level interface of
 * three Cython `cdef class`es and one NumPy loop.  Each group of entry points below replaces one of them;
 * the reference interface it stands in for is cited as file:line (relative to the reference root).  The
 * ctypes stub a maintainer would add on the reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, a negative MI355REC_E_* code otherwise;
 *     mi355rec_last_error() returns a thread-local human-readable message for the last failure;
 *   - host buffers are owned by the caller and only read/written for the duration of the call;
 *     *_create copies its inputs to HBM; handles own device memory and one HIP stream;
 *   - pointers named d_* are DEVICE pointers (e.g. torch tensor .data_ptr()), everything else is host;
 *   - all calls are blocking unless stated; one handle must not be used from two threads at once;
 *   - the HIP context is created lazily by the first *_create in the calling process (fork-safe import);
 *   - indices are int32, values float32; CSR rows must have sorted column indices.
 */
#ifndef MI355REC_H
#define MI355REC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355REC_OK              0
#define MI355REC_E_INVALID      -1   /* bad argument (maps to ValueError on the Python side) */
#define MI355REC_E_HIP          -2   /* HIP runtime failure */
#define MI355REC_E_NO_DEVICE    -3   /* no gfx950 device visible */
#define MI355REC_E_UNSUPPORTED  -4   /* valid in the reference, not (yet) covered by the device path */
#define MI355REC_E_NUMERIC      -5   /* non-finite value / not positive definite */

const char *mi355rec_last_error(void);

/* Raw device buffers of the calling process's device, for callers that keep results on the GPU and exchange them between
 * GPUs themselves (sharding.py: RCCL all-gather of similarity slabs through ctypes, no PyTorch).  to_device: 1 = host -> device,
 * 0 = device -> host, 2 = device -> device; the copies are blocking. */
int mi355rec_device_malloc(void **out, uint64_t bytes);
int mi355rec_device_free(void *p);
int mi355rec_device_memcpy(void *dst, const void *src, uint64_t bytes, int to_device);
int mi355rec_device_synchronize(void);
/* Device blocks that handles have released stay in a per-process cache (hipFree drains the device and costs 0.2 - 0.5 ms per block: a
 * dozen temporaries made up a third of a similarity constructor); at most MI355REC_POOL_BYTES of them (default 8 GiB of the device's 288, 0: no cache).
 * mi355rec_device_trim gives every cached block back to the driver -- for a process that shares the device with another allocator
 * (PyTorch, RCCL) and is done with a phase of fits; *freed_bytes (nullable) receives what was returned. */
int mi355rec_device_trim(uint64_t *freed_bytes);
/* Number of visible HIP devices (0 and MI355REC_OK when none). */
int mi355rec_device_count(int *count);
/* Select the device used by handles created afterwards in this process (one process per GPU: LOCAL_RANK). */
int mi355rec_set_device(int device);
/* "gfx950:..." architecture string of the current device. */
int mi355rec_device_name(char *buf, int buf_len);

/* Timing of the last run/compute call on a handle, measured with HIP events on the handle's own stream
 * (bench.py's throughput and roofline figures come from here).
 *   call_ms    events recorded on the stream immediately before the first and after the last kernel of the call;
 *   kernel_ms  SUM of the durations of the timed launches of the DOMINANT kernel (mf: gradient kernel, sim: column
 *              kernel, slim: step kernel, ials: row-solve kernel), each measured by the start/stop events the
 *              dispatch itself carries (hipExtLaunchKernelGGL) -- the same begin/end timestamps rocprofv3
 *              --kernel-trace reports; n_timed of the n_launches launches were timed (see *_set_profiling). */
typedef struct {
    double  call_ms;
    double  kernel_ms;
    int64_t n_launches;     /* launches of the dominant kernel in the call */
    int64_t n_timed;        /* how many of them carry timing events (kernel_ms / n_timed = average launch duration) */
    int64_t n_units;        /* units processed: samples (mf, slim), columns (sim), row solves (ials) */
    double  algorithmic_bytes; /* ALGORITHMIC bytes of the WHOLE call (definition: DESIGN.md section 4) */
    double  algorithmic_flops; /* ALGORITHMIC flops of the whole call (ials), 0 elsewhere */
    double  loss;           /* cumulative x_uij^2 / squared error of the call where defined, else 0 */
} mi355rec_stats;

/* ------------------------------------------------------------------------------------------------------
 * Compute_Similarity  (Base/Similarity/Cython/Compute_Similarity_Cython.pyx:51  cdef class
 * Compute_Similarity_Cython; __init__ :72-213; compute_similarity(start_col, end_col) :411-607)
 * ---------------------------------------------------------------------------------------------------- */

enum {                       /* `similarity=` strings of Compute_Similarity_Cython.__init__ (.pyx:118-143) */
    MI355REC_SIM_COSINE     = 0,
    MI355REC_SIM_ADJUSTED   = 1,
    MI355REC_SIM_ASYMMETRIC = 2,
    MI355REC_SIM_PEARSON    = 3,
    MI355REC_SIM_JACCARD    = 4,   /* == "tanimoto" */
    MI355REC_SIM_DICE       = 5,
    MI355REC_SIM_TVERSKY    = 6,
    MI355REC_SIM_EUCLIDEAN  = 7    /* Base/Similarity/Compute_Similarity_Euclidean.py:16 (reached through the dispatcher,
                                    * Compute_Similarity.py:59-62): 1 / (f(distance) + shrink + 1e-9), float32 arithmetic */
};

enum {                       /* `similarity_from_distance_mode=` of Compute_Similarity_Euclidean (:46-57, :189-196) */
    MI355REC_EUCLID_LIN = 0, /* f(d) = d         */
    MI355REC_EUCLID_LOG = 1, /* f(d) = log(d+1)  */
    MI355REC_EUCLID_EXP = 2  /* f(d) = exp(d)    */
};

typedef struct {
    int32_t topK;            /* 0 = dense output only (.pyx:507-510); clamped to n_cols like .pyx:146 */
    int32_t shrink;          /* already truncated to int, as `cdef int shrink` does (.pyx:64) */
    int32_t normalize;
    int32_t similarity;      /* MI355REC_SIM_* */
    float   asymmetric_alpha, tversky_alpha, tversky_beta;   /* `cdef float` in the reference (.pyx:65) */
    int32_t unit_column_side;   /* 1: the value of (row u, column c) on the COLUMN side of the product is taken as 1, i.e.
                                 * out(c, j) = sum over the rows u storing c of data[u, j] -- the boolean-transpose product of
                                 * the graph recommenders (GraphBased/P3alphaRecommender.py:69-104); 0: the plain self-product */
    int32_t normalize_avg_row;  /* MI355REC_SIM_EUCLIDEAN only: squared distance divided by n_rows (Euclidean.py:181-182);
                                 * `normalize` then means squared distance / (|a| |b|) (:178-179) */
    int32_t euclidean_mode;     /* MI355REC_EUCLID_* */
    /* Optional pre-pass: the BM25 / TF-IDF re-weighting the KNN recommenders apply to the matrix before the build
     * (Base/IR_feature_weighting.py:13 okapi_BM_25, :55 TF_IDF; KNN/ItemKNNCFRecommender.py:40-48, UserKNNCFRecommender.py:40-48),
     * on the stored values already in HBM.  "Documents" are the rows of the matrix the reference hands to those functions:
     * for ItemKNN (URM.T weighted, URM built) the COLUMNS of dataMatrix, for UserKNN (URM.T weighted, URM.T built) its ROWS. */
    int32_t feature_weighting;      /* MI355REC_WEIGHT_* */
    int32_t weighting_documents;    /* 0: documents = columns of dataMatrix, 1: documents = rows */
    float   bm25_k1, bm25_b;        /* okapi_BM_25(K1 = 1.2, B = 0.75) */
    /* How the reference sums the squares behind the column norms, `dataMatrix.power(2).sum(axis=0)` (.pyx:169,
     * Compute_Similarity_Euclidean.py:112): in the matrix's own dtype -- float32 for a URM -- and in an ORDER that depends on the
     * sparse format SciPy finds: a CSR matrix is summed as ones @ X, i.e. every column's squares are added one after the other in
     * row order into a float32 (heavy columns of jittered ratings lose 2e-4 of their norm that way), a CSC matrix by
     * np.add.reduceat, i.e. first square + NumPy's pairwise float32 sum of the rest.  0: the CSR order (also adjusted cosine,
     * whose pre-pass returns CSR, .pyx:275); 1: the CSC order (also pearson, whose pre-pass returns CSC, .pyx:234). */
    int32_t norm_sum_order;
    int32_t reserved;
} mi355rec_sim_config;

enum { MI355REC_WEIGHT_NONE = 0, MI355REC_WEIGHT_BM25 = 1, MI355REC_WEIGHT_TFIDF = 2 };

typedef struct mi355rec_sim *mi355rec_sim_t;

/* dataMatrix (n_rows x n_cols) as CSR; similarities are computed between its COLUMNS.  row_weights is
 * nullable (length n_rows; with MI355REC_SIM_EUCLIDEAN it needs n_rows == n_cols, Compute_Similarity_Euclidean.py:174-175, else
 * MI355REC_E_INVALID).  Pre-processing (mean-centring / binarisation / column norms, .pyx:153-192),
 * the CSR->CSC transposition (.pyx:198-207) and the cost-ordered column schedule are done on the device. */
int mi355rec_sim_create(mi355rec_sim_t *out, const mi355rec_sim_config *cfg, int32_t n_rows, int32_t n_cols,
                        const int32_t *csr_indptr, const int32_t *csr_indices, const float *csr_data,
                        const float *row_weights);
/* The same constructor for a dataMatrix that is ALREADY in device memory (d_* are device pointers of the calling process's GPU;
 * row_weights stays a host array): the handle copies the three arrays at HBM speed instead of uploading 8 B per stored value over
 * PCIe -- 2.9 of the 6.7 ms the constructor takes at ML-20M shape.  The reference's hyper-parameter search fits hundreds of models
 * on one URM_train (ParameterTuning/SearchAbstractClass.py:253-262, one `fit` per configuration): the matrix is uploaded once
 * (`ResidentURM` in the Python front-end) and every ItemKNN fit starts from the resident copy (P3alpha / RP3beta build from a
 * row-normalised, re-weighted matrix of their own and upload that).  The caller keeps
 * ownership of the arrays; they are not modified and may be freed as soon as the call returns. */
int mi355rec_sim_create_resident(mi355rec_sim_t *out, const mi355rec_sim_config *cfg, int32_t n_rows, int32_t n_cols,
                                 const int32_t *d_csr_indptr, const int32_t *d_csr_indices, const float *d_csr_data,
                                 const float *row_weights);
/* Multi-GPU partition with equal column COUNTS and equal COST per part: the columns in cost order are dealt to n_parts parts in
 * serpentine order; part `part` computes its columns and writes column mi355rec_sim_part_columns()[q] to row q of the
 * DEVICE slabs (ceil(n_cols / n_parts) x topK each).  Same kernel as mi355rec_sim_compute_device; the contiguous
 * [start_col, end_col) entry points keep the reference's own seam (Compute_Similarity_Cython.pyx:411, 447-451). */
int mi355rec_sim_compute_part_device(mi355rec_sim_t h, int32_t part, int32_t n_parts, int32_t *d_nbr_idx, float *d_nbr_val);
/* The same for rows [slot_first, slot_first + slot_count) of the part only, written to rows 0 .. slot_count - 1 of the slabs handed
 * in: a sharded build computes its part in chunks so that the all-gather of a finished chunk travels while the next one is built. */
int mi355rec_sim_compute_part_chunk_device(mi355rec_sim_t h, int32_t part, int32_t n_parts, int32_t slot_first, int32_t slot_count,
                                           int32_t *d_nbr_idx, float *d_nbr_val);
/* The exchange format of the sharded build when n_cols <= 65 535 (6 bytes per neighbour instead of 8): n_cells float32 values followed by
 * n_cells 16-bit neighbour ids (0xFFFF = the -1 of an empty slot), padded to a multiple of 4 bytes -- n_cells + (n_cells + 1) / 2 words.
 * pack: from the (idx, val) slabs a compute_*_device call filled; unpack: back into such slabs.  Asynchronous on the handle's stream.
 * What travels is what Compute_Similarity_Cython.pyx:593-607 would assemble into W_sparse on one process. */
int mi355rec_sim_pack_slab_device(mi355rec_sim_t h, const int32_t *d_nbr_idx, const float *d_nbr_val, int64_t n_cells, void *d_packed);
int mi355rec_sim_unpack_slab_device(mi355rec_sim_t h, const void *d_packed, int64_t n_cells, int32_t *d_nbr_idx, float *d_nbr_val);
/* The columns of a part in output-row order (columns may be NULL: only the count). */
int mi355rec_sim_part_columns(mi355rec_sim_t h, int32_t part, int32_t n_parts, int32_t *columns, int32_t *n_columns);
/* The re-weighted stored values (feature_weighting != NONE), in the order of the csr_data passed to mi355rec_sim_create: what the
 * reference recommender keeps as its URM_train afterwards (ItemKNNCFRecommender.py:42-43). */
int mi355rec_sim_get_weighted_values(mi355rec_sim_t h, float *csr_data);
/* Columns [start_col, end_col): for local column c the topK (neighbour, value) pairs in descending value
 * order at nbr_idx/nbr_val[(c - start_col) * topK ...], padded with (-1, 0).  Zero similarities are never
 * emitted (.pyx:555). */
int mi355rec_sim_compute(mi355rec_sim_t h, int32_t start_col, int32_t end_col, int32_t *nbr_idx, float *nbr_val);
/* Same, results left in device memory (for the RCCL gather of the column-sharded build); asynchronous on
 * the handle's stream -- call mi355rec_sim_sync before another stream/library reads the buffers. */
int mi355rec_sim_compute_device(mi355rec_sim_t h, int32_t start_col, int32_t end_col, int32_t *d_nbr_idx, float *d_nbr_val);
/* Same columns, assembled on the device into the CSR matrix the reference returns (.pyx:603-605): row = neighbour,
 * column = source item, column indices ascending inside a row.  indptr: n_cols + 1; indices / data: capacity
 * (end_col - start_col) * topK, the first *nnz entries are written.  (The host-side COO -> CSR conversion of 2.7 M cells
 * takes ~200 ms in SciPy -- more than ten times the whole device build at ML-20M shape.) */
int mi355rec_sim_compute_csr(mi355rec_sim_t h, int32_t start_col, int32_t end_col, int32_t *indptr, int32_t *indices,
                             float *data, int64_t *nnz);
/* topK == 0 variant (.pyx:507-510): W[j * ld + (c - start_col)] = similarity(j, c); W is host, row-major, ld >= end_col-start_col. */
int mi355rec_sim_compute_dense(mi355rec_sim_t h, int32_t start_col, int32_t end_col, float *W, int64_t ld);
/* The same columns left on the device: column c contiguous at d_W + (c - start_col) * ld (ld >= n_cols); nothing is downloaded.
 * Returns after the handle's stream has drained. */
int mi355rec_sim_compute_dense_device(mi355rec_sim_t h, int32_t start_col, int32_t end_col, float *d_W, int64_t ld);
/* cost(c) = sum over users of column c of their profile length: the work of one column; used to cut
 * cost-balanced column ranges for multi-GPU sharding. */
int mi355rec_sim_column_costs(mi355rec_sim_t h, int64_t *cost /* n_cols */);
/* Schedule of the last compute call: work items queued, columns that were split over several workgroups, and the
 * number of parts they were split into (diagnostics; a heavy column is accumulated by several workgroups). */
int mi355rec_sim_schedule_info(mi355rec_sim_t h, int32_t *n_items, int32_t *n_split_columns, int32_t *n_parts);
/* Type of the in-LDS column accumulator this handle's builds use: 0 = uint32 co-occurrence counts (all stored values 1.0, no
 * row_weights), 3 = exact int32 sums (every stored value times 2^s, s <= 3, is a small integer -- star ratings, half stars -- and no
 * row_weights / mean-centring: the products scaled by *fixed_scale = 4^s are integers; MI355REC_SIM_NO_INT32=1 disables it),
 * 1 = int64 fixed point (real-valued data whose products, scaled by the power of two *fixed_scale, keep every sum
 * inside 62 bits with a worst-case rounding below 1e-6 of the smallest normalised result), 2 = float64 sums like the reference's
 * double array (Compute_Similarity_Cython.pyx:363; chosen when no such scale exists, or with MI355REC_SIM_F64_SUMS=1 in the
 * environment at create time).  Diagnostics for the parity tests. */
int mi355rec_sim_accumulator_info(mi355rec_sim_t h, int32_t *kind, double *fixed_scale);
/* Selection path of the last compute call (diagnostics for the parity tests): columns whose top-K was found threshold-first
 * (per-thread maxima -> K-th largest maximum -> exact division of the survivors only; csrc/sim_kernels.cuh), the survivors those columns
 * ranked in total, and columns that went back to the full normalise + radix select after their scan (more survivors than the
 * candidate buffer holds).  Columns with fewer than topK positive cells, accumulator tiles, 8-byte cells, topK == 0 and the
 * Euclidean cell map always take the full path and are counted nowhere.  MI355REC_SIM_FAST_TOPK=0 switches the first path off. */
int mi355rec_sim_selection_info(mi355rec_sim_t h, int64_t *threshold_first_columns, int64_t *candidates, int64_t *fallbacks);
int mi355rec_sim_sync(mi355rec_sim_t h);
/* The rate the column kernel's accumulation is priced against (bench.py's `roofline.peak` of the ItemKNN build), measured on the device at
 * hand: ds_add_u32 lane-adds per second of the whole device on uniformly random cells of a 128 KiB LDS array, one 1024-thread workgroup
 * per CU (the loop of scripts/micro/lds_atomics.hip).  ~10 ms. */
int mi355rec_lds_atomic_rate(double *lane_adds_per_second);
int mi355rec_sim_get_stats(mi355rec_sim_t h, mi355rec_stats *stats);
void mi355rec_sim_destroy(mi355rec_sim_t h);

/* ------------------------------------------------------------------------------------------------------
 * Stacking CSR matrices that are already in device memory (csrc/stack.hip): the dataMatrix of the CF+CBF hybrid KNN
 * recommenders (KNN/ItemKNN_CFCBF_Hybrid_Recommender.py:20-25: hstack([ICM_train * ICM_weight, URM_train.T]), built on its
 * transpose) is a few feature rows on top of the user rows.  The blocks stay resident for a whole search; only the weight changes
 * from fit to fit, so the stack is made in HBM and handed to mi355rec_sim_create_resident.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_rows;             /* rows of the block (0 is allowed) */
    int32_t nnz;                /* stored cells of the block */
    const int32_t *d_indptr;    /* n_rows + 1 row pointers starting at 0 (device) */
    const int32_t *d_indices;   /* nnz column ids in [0, n_cols) (device; may be NULL when nnz == 0) */
    const float *d_data;        /* nnz values (device; may be NULL when nnz == 0) */
    float scale;                /* every value of the block is multiplied by it, one float32 product (NumPy's `data * w` of a
                                 * float32 array); exactly 1 copies the bits */
} mi355rec_csr_block;

#define MI355REC_STACK_MAX_BLOCKS 16

/* d_indptr (total rows + 1), d_indices and d_data (total cells each): the CSR of the blocks' rows one after the other -- row
 * pointers offset by the cells of the blocks before, indices copied, values scaled.  One launch for all blocks and arrays; returns
 * after it has run.  Checked on the host before anything touches the device (MI355REC_E_INVALID): n_blocks < 1, NULL arguments,
 * negative sizes, total rows or total cells beyond int32; more than MI355REC_STACK_MAX_BLOCKS blocks is MI355REC_E_UNSUPPORTED.  A
 * column id outside [0, n_cols) found while copying is MI355REC_E_INVALID as well (the outputs are then not to be used). */
int mi355rec_csr_stack_device(int32_t n_blocks, const mi355rec_csr_block *blocks, int32_t n_cols, int32_t *d_indptr,
                              int32_t *d_indices, float *d_data);

/* ------------------------------------------------------------------------------------------------------
 * Matrix-factorisation SGD epochs  (MatrixFactorization/Cython/MatrixFactorization_Cython_Epoch.pyx:50
 * cdef class MatrixFactorization_Cython_Epoch; __init__ :95-148; epochIteration_Cython :273;
 * get_USER_factors ... get_GLOBAL_bias :685-702)
 * ---------------------------------------------------------------------------------------------------- */

enum { MI355REC_MF_BPR = 0, MI355REC_MF_FUNK_SVD = 1, MI355REC_MF_ASY_SVD = 2 };   /* algorithm_name (.pyx:93) */
enum { MI355REC_SGD = 0, MI355REC_ADAGRAD = 1, MI355REC_RMSPROP = 2, MI355REC_ADAM = 3 };  /* sgd_mode (.pyx:92) */
enum { MI355REC_F32 = 0, MI355REC_F64 = 1 };

typedef struct {
    int32_t algorithm;       /* MI355REC_MF_* */
    int32_t n_factors;
    int32_t batch_size;
    int32_t use_bias;
    int32_t sgd_mode;        /* MI355REC_SGD ... */
    /* hyper-parameters are double like the reference's `cdef double` attributes (.pyx:55-56): derived constants
     * such as (1 - gamma) = 0.005 must not be formed from float-rounded inputs */
    double  learning_rate;
    double  user_reg, item_reg, bias_reg, positive_reg, negative_reg;
    double  negative_interactions_quota;
    double  gamma, beta_1, beta_2;
    uint64_t random_seed;    /* seeds the on-device counter-based sampler */
    int32_t precision;       /* MI355REC_F32 / MI355REC_F64: storage AND arithmetic type of factors, biases and optimiser
                              * moments on the device, and the element type of U0 / V0.  The reference computes in double
                              * (.pyx:55-66); float32 holds the 1e-5 bar for plain sgd, the adaptive optimisers divide
                              * every gradient component by sqrt(running g^2) + 1e-8 and need float64 state for it. */
    int32_t reserved;
} mi355rec_mf_config;

typedef struct mi355rec_mf *mi355rec_mf_t;

/* URM (n_users x n_items) as CSR with sorted indices.  U0 (n_users x k; n_ITEMS x k for ASY_SVD, whose "user" matrix is
 * the second item-sized matrix Y, .pyx:163-166) and V0 (n_items x k) are the initial factors, row-major, float32 or float64
 * as cfg->precision says (the host draws them exactly like .pyx:174-175 does).  ASY_SVD requires batch_size == 1 (.pyx:395) and runs its nnz + 1 steps per
 * epoch strictly in order. */
int mi355rec_mf_create(mi355rec_mf_t *out, const mi355rec_mf_config *cfg, int32_t n_users, int32_t n_items,
                       const int32_t *indptr, const int32_t *indices, const float *data,
                       const void *U0, const void *V0);
/* n_epochs x epochIteration_Cython(): each epoch is n_users/B+1 (BPR, .pyx:583) or nnz/B+1 (FunkSVD, :289)
 * mini-batches of B samples drawn ON THE DEVICE. */
int mi355rec_mf_run_epochs(mi355rec_mf_t h, int32_t n_epochs);
/* Parity mode: the same arithmetic on a caller-provided sample stream, cut into consecutive mini-batches of
 * batch_size (the last one may be short but is still averaged over batch_size, like .pyx:802).
 * BPR: (u, i, j); FunkSVD: (u, i, rating) with j == NULL.  A user id outside [0, n_users) or an item id outside
 * [0, n_items) is MI355REC_E_INVALID: nothing is copied or run. */
int mi355rec_mf_run_samples(mi355rec_mf_t h, const int32_t *u, const int32_t *i, const int32_t *j,
                            const float *rating, int64_t n);
/* Exact multi-GPU mini-batches (MF_BPR with sgd): one epoch with the tasks of every mini-batch split over
 * `world` identical replicas -- same URM, same initial factors, same random_seed, hence the same on-device sample stream and
 * schedule.  Rank `rank` computes the new version of the rows owned by its share of a mini-batch's tasks
 * (mi355rec_mf_shard_batch: kernel + packing of those rows into *d_send, blocking); the caller all-gathers *d_send
 * (bytes_per_rank) into *d_recv (world x bytes_per_rank: ncclAllGather / all_gather_into_tensor); mi355rec_mf_shard_merge copies
 * the other ranks' rows in (blocking).  After every merge all replicas hold bit-identical factors, equal to a single-GPU
 * epoch's.  One exchange per mini-batch: only pays for large batch_size.  */
int mi355rec_mf_shard_begin_epoch(mi355rec_mf_t h, int32_t rank, int32_t world, void **d_send, void **d_recv,
                                  uint64_t *bytes_per_rank, int32_t *n_batches);
int mi355rec_mf_shard_batch(mi355rec_mf_t h, int32_t batch);
int mi355rec_mf_shard_merge(mi355rec_mf_t h, int32_t batch);
int mi355rec_mf_shard_end_epoch(mi355rec_mf_t h);
/* Any output pointer may be NULL.  bu/bi/mu are only written when use_bias. */
int mi355rec_mf_get_factors(mi355rec_mf_t h, float *U, float *V, float *bu, float *bi, float *mu);
/* The same as float64, the type the reference's getters return (.pyx:685-702): the device state itself when it is float64
 * (adagrad / rmsprop / adam, AsySVD), the float32 state widened otherwise. */
int mi355rec_mf_get_factors_f64(mi355rec_mf_t h, double *U, double *V, double *bu, double *bi, double *mu);
/* AsySVD's user factors from the handle's own URM and its Y, on the device (MatrixFactorization_Cython.py:281-304,
 * _estimate_user_factors): out[u, f] = (sum over the profile of u, in the handle's storage order -- sorted ids -- of
 * (double)rating * Y[item, f]) / row_divisor[u], SciPy's csr_matvecs recurrence in float64 bit for bit (every product and every sum
 * rounded on its own, starting from +0.0) and one IEEE division.  row_divisor (n_users, host) is the caller's:
 * sqrt(profile length) computed on the host; a row whose divisor is not above 0 is left undivided, +0.0 for an empty profile.
 * out is n_users x k float64 on the host.  Queued on the handle's stream behind its training work; the handle's state is not
 * changed.  MI355REC_E_UNSUPPORTED for a handle that is not ASY_SVD or whose state is float32.
 * Stats: kernel_ms the one launch, call_ms with the copies around it, algorithmic_bytes = nnz (8 k + 8) + 8 n_users k. */
int mi355rec_mf_asy_user_factors(mi355rec_mf_t h, const double *row_divisor, double *out);
/* The same without a handle (the cold users of a new URM, after the training handle is closed): uploads, runs the same kernel,
 * downloads.  Rows are summed in the order they are stored, sorted or not.  Y is n_items x k float64, k as an ASY_SVD handle takes
 * it.  Row pointers that do not climb from 0, or a column id outside [0, n_items), are MI355REC_E_INVALID: nothing is run and out
 * is not written. */
int mi355rec_asy_user_factors(int32_t n_rows, int32_t n_items, int32_t k, const int32_t *indptr, const int32_t *indices,
                              const float *data, const double *Y, const double *row_divisor, double *out);
/* Copy the (u, i, j|rating) stream drawn by the LAST mi355rec_mf_run_epochs call (at most cap entries);
 * returns the number of samples of that call in *n. */
int mi355rec_mf_get_last_samples(mi355rec_mf_t h, int32_t *u, int32_t *i, int32_t *j, float *rating, int64_t cap, int64_t *n);
/* Time (at most) the first max_timed_launches mini-batch kernel launches of every subsequent call with per-dispatch
 * events; 0 (default) disables it. */
int mi355rec_mf_set_profiling(mi355rec_mf_t h, int32_t max_timed_launches);
/* Diagnostics (handles created with MI355REC_MF_TICKS=1 in the environment): shader-clock stamps of every wavefront of the
 * LAST mini-batch run, 8 words per task slot {entry, header arrived, first rows arrived, list done, exit, list length,
 * own row written, taken-over item rows written}.  *n receives the number of words available (0 when the handle was created without the variable). */
int mi355rec_mf_get_phase_ticks(mi355rec_mf_t h, uint64_t *out, int64_t cap, int64_t *n);
/* The same for the in-LDS schedule's sort kernel, last schedule built: 8 words per mini-batch, stamped by thread 0 of its workgroup
 * {entry, keys in LDS (drawn or read back), sorted, run heads, once-touched flags, slot scans, headers written, exit}. */
int mi355rec_mf_get_schedule_ticks(mi355rec_mf_t h, uint64_t *out, int64_t cap, int64_t *n);
int mi355rec_mf_get_stats(mi355rec_mf_t h, mi355rec_stats *stats);
void mi355rec_mf_destroy(mi355rec_mf_t h);

/* Replica-batched epochs: R independent models trained side by side, the way the reference's hyper-parameter search runs this
 * path (ParameterTuning/run_parameter_search.py:498-503: a multiprocessing Pool, one model per worker; each worker's fit() is a
 * loop over MatrixFactorization_Cython_Epoch.epochIteration_Cython, MatrixFactorization_Cython.py:126).  One epoch of ONE model
 * is a chain of dependent mini-batches of ~3 MB each, which fills a tenth of an MI355X; a group launches mini-batch b of ALL
 * members as one grid, so the chain keeps its length and every link moves R mini-batches.  Members are ordinary handles
 * (not owned by the group, usable on their own between group calls, each with its own factors, hyper-parameters, optimiser,
 * seed and sample stream); they must share what a launch shares: algorithm (MF_BPR or FUNK_SVD), precision, batch_size, the
 * number of mini-batches per epoch and the kernel instance n_factors selects (float32: n_factors % 4 == 0 and <= 64 / <= 128 /
 * <= 256 / <= 512; float64: % 2 and half those bounds).  Every member ends bit-identical to running its epochs alone. */
typedef struct mi355rec_mf_group *mi355rec_mf_group_t;
int mi355rec_mf_group_create(mi355rec_mf_group_t *out, const mi355rec_mf_t *members, int32_t n_members);
/* n_epochs x epochIteration_Cython() of every member (blocking).  Afterwards each member's get_factors / get_last_samples /
 * get_stats (n_units, loss of ITS samples) answer as after its own run_epochs call. */
int mi355rec_mf_group_run_epochs(mi355rec_mf_group_t g, int32_t n_epochs);
int mi355rec_mf_group_set_profiling(mi355rec_mf_group_t g, int32_t max_timed_launches);
/* call_ms / kernel_ms of the last call; n_units, algorithmic_bytes and loss summed over the members. */
int mi355rec_mf_group_get_stats(mi355rec_mf_group_t g, mi355rec_stats *stats);
void mi355rec_mf_group_destroy(mi355rec_mf_group_t g);     /* the members stay alive */

/* ------------------------------------------------------------------------------------------------------
 * SLIM-BPR epoch  (SLIM_BPR/Cython/SLIM_BPR_Cython_Epoch.pyx:59 cdef class SLIM_BPR_Cython_Epoch;
 * __init__ :87-135; epochIteration_Cython :212; get_S :343-391; _dealloc :195)
 * ---------------------------------------------------------------------------------------------------- */

typedef struct {
    int32_t symmetric;       /* 1: S[i,s] aliases S[s,i] (Triangular_Matrix, .pyx:1290-1330) */
    int32_t sgd_mode;
    double  learning_rate, li_reg, lj_reg;
    double  gamma, beta_1, beta_2;
    uint64_t random_seed;
    int32_t precision;       /* MI355REC_F32 / MI355REC_F64: type of the dense store's cells and per-item optimiser cells on the device
                              * (the reference is double throughout).  Rows an owning workgroup keeps in LDS for a launch are float32
                              * there; the symmetric store holds float32 values in 8-byte {value, tag} cells, computes in float64
                              * and keeps the optimiser cells as float64 (two float32 halves) whatever this field says */
    int32_t train_with_sparse_weights;   /* 1: the semantics of the Sparse_Matrix_Tree_CSR store (.pyx:582-1030) on the dense
                              * device array: a cell "has a node" once it has been written; rebalance_tree(TopK) (.pyx:320-324,
                              * 785-805) keeps the TopK largest nodes per row after every (n_steps / 5)-th step of an epoch, get_S
                              * selects once more and keeps the selection (.pyx:381-382, 740-780).  Forces symmetric = 0
                              * (.pyx:112-113) and needs MI355REC_F64 */
    int32_t topK;            /* sparse store only: the TopK of the selections; 0 = the reference's `topK = False` (no selection) */
    int32_t reserved;
} mi355rec_slim_config;

typedef struct mi355rec_slim *mi355rec_slim_t;

int mi355rec_slim_create(mi355rec_slim_t *out, const mi355rec_slim_config *cfg, int32_t n_users, int32_t n_items,
                         const int32_t *indptr, const int32_t *indices);
/* n_epochs x epochIteration_Cython() with the wrapper's batch_size = 1 (SLIM_BPR_Cython.py:140): n_users+1
 * strictly ordered samples per epoch, drawn on the device and executed in stream order. */
int mi355rec_slim_run_epochs(mi355rec_slim_t h, int32_t n_epochs);
int mi355rec_slim_run_samples(mi355rec_slim_t h, const int32_t *u, const int32_t *i, const int32_t *j, int64_t n);
/* The (u, i, j) stream of the LAST epoch drawn on the device (at most cap entries; *n = its length, 0 before the first epoch). */
int mi355rec_slim_get_last_samples(mi355rec_slim_t h, int32_t *u, int32_t *i, int32_t *j, int64_t cap, int64_t *n);
/* get_S: diagonal zeroed, per-ROW top-K (.pyx:343-391): nbr_idx/nbr_val[(row) * topK ...], descending,
 * (-1, 0) padded, zeros never emitted. */
int mi355rec_slim_get_S_topk(mi355rec_slim_t h, int32_t topK, int32_t *nbr_idx, float *nbr_val);
/* W_sparse = similarityMatrixTopK(get_S(), k = topK) (SLIM_BPR_Cython.py:186-197 at every validation; Base/Recommender_utils.py:55-122): of
 * the per-row selection above, every COLUMN keeps its topK largest non-zero cells (of equal values the highest rows, as the reference's
 * stable ascending sort leaves them), returned as canonical CSR (indptr [n_items + 1], indices / data with room for n_items * topK
 * entries, *nnz = how many were written).  nbr_idx / nbr_val (optional, may be NULL): the row slabs of mi355rec_slim_get_S_topk from
 * the same pass.  n_items <= 65 535. */
int mi355rec_slim_get_W_csr(mi355rec_slim_t h, int32_t topK, int32_t *nbr_idx, float *nbr_val, int32_t *indptr, int32_t *indices,
                            float *data, int64_t *nnz);
/* get_S of the sparse store with topK > 0 (.pyx:343-352, 381-382): the diagonal becomes a node holding zero, every row keeps
 * its TopK largest nodes (the model changes, as in the reference), and the surviving NON-ZERO nodes of row r are listed in
 * column order in nbr_idx/nbr_val[r * topK ...], (-1, 0) padded (from_linked_list_to_python_list :862-875). */
int mi355rec_slim_get_S_sparse(mi355rec_slim_t h, int32_t *nbr_idx, float *nbr_val);
/* Dense S (n_items x n_items, row-major, diagonal zeroed, symmetric mode mirrored). */
int mi355rec_slim_get_S_dense(mi355rec_slim_t h, float *S);
int mi355rec_slim_get_stats(mi355rec_slim_t h, mi355rec_stats *stats);
/* Diagnostics of the last dense-store launch: rows kept in the LDS of an owning workgroup (the busiest items of the stream; 0 on
 * the symmetric / sparse store, for catalogues whose row does not fit the LDS, or when no compute units could be leased) and the
 * number of steps that ran on rows in HBM. */
int mi355rec_slim_schedule_info(mi355rec_slim_t h, int32_t *n_owned_rows, int32_t *n_cold_steps);
void mi355rec_slim_destroy(mi355rec_slim_t h);

/* ------------------------------------------------------------------------------------------------------
 * IALS solve step  (MatrixFactorization/IALSRecommender.py:137 _run_epoch, :170 _update_row)
 * ---------------------------------------------------------------------------------------------------- */

typedef struct mi355rec_ials *mi355rec_ials_t;

/* C (confidence, n_users x n_items) as CSR with float32 data = 1 + alpha*r etc. (IALSRecommender.py:111-123,
 * computed by the host exactly as the reference does).  V0: initial item factors (n_items x k); U0: initial
 * user factors (only cold users keep them; nullable = zeros). */
int mi355rec_ials_create(mi355rec_ials_t *out, int32_t n_users, int32_t n_items, int32_t n_factors, double reg,
                         const int32_t *indptr, const int32_t *indices, const float *confidence,
                         const double *U0, const double *V0);
/* Restrict the row solves of subsequent epochs to users [u0,u1) and items [i0,i1) (multi-GPU sharding);
 * the caller all-gathers the factor shards between the two half-steps through the *_half entry points. */
int mi355rec_ials_run_epochs(mi355rec_ials_t h, int32_t n_epochs);
int mi355rec_ials_user_half(mi355rec_ials_t h, int32_t u0, int32_t u1);
int mi355rec_ials_item_half(mi355rec_ials_t h, int32_t i0, int32_t i1);
/* Device pointers to the float64 factor matrices (n_users x k, n_items x k), for the RCCL all-gather. */
int mi355rec_ials_device_factors(mi355rec_ials_t h, double **d_U, double **d_V);
int mi355rec_ials_sync(mi355rec_ials_t h);
int mi355rec_ials_get_factors(mi355rec_ials_t h, double *U, double *V);
/* Schedule of the last half-step: rows whose Gramian was split over several workgroups (profiles longer than 8192 entries: parts of
 * 4096, the last arriver adds the parts up in part order and solves) and the number of parts (diagnostics). */
int mi355rec_ials_schedule_info(mi355rec_ials_t h, int32_t *n_split_rows, int32_t *n_parts);
int mi355rec_ials_get_stats(mi355rec_ials_t h, mi355rec_stats *stats);
void mi355rec_ials_destroy(mi355rec_ials_t h);

/* ------------------------------------------------------------------------------------------------------
 * SLIM ElasticNet  (SLIM_ElasticNet/SLIMElasticNetRecommender.py:41-149: one sklearn ElasticNet per item, sparse coordinate
 * descent with selection='random', _cd_fast.pyx sparse_enet_coordinate_descent) as coordinate descent on the Gram matrix
 * ---------------------------------------------------------------------------------------------------- */

typedef struct mi355rec_slimen *mi355rec_slimen_t;

/* URM_train (n_users x n_items) in both layouts, CSR and CSC, float32 values, sorted indices.  Builds G = X^T X (n_items^2 float32,
 * kept on the device; the fits read it there and mi355rec_slimen_get_gram copies rows of it out) and diag = column sums of squares;
 * fails with MI355REC_E_INVALID when G does not fit the free memory.  Row j of G is accumulated in LDS up to 40 960 items and by global
 * atomics into the row itself beyond; MI355REC_SLIMEN_GLOBAL_GRAM=1 forces the latter at any size (tests). */
int mi355rec_slimen_create(mi355rec_slimen_t *out, int32_t n_users, int32_t n_items, const int32_t *row_ptr, const int32_t *row_idx,
                           const float *row_val, const int32_t *col_ptr, const int32_t *col_idx, const float *col_val);
/* Fits the targets [start_item, end_item): seeds[t] is the solver seed of target start_item + t (np.random.randint(0, 2**31 - 1),
 * drawn by the caller in item order); alpha, l1_ratio, positive, max_iter and tol as sklearn's ElasticNet (l1 = alpha * l1_ratio *
 * n_users, l2 = alpha * (1 - l1_ratio) * n_users); topK: per target the min(nnz - 1, topK) largest coefficients are kept
 * (SLIMElasticNetRecommender.py:107-111); topK = -1 keeps every nonzero coefficient (diagnostics: the whole solution). */
int mi355rec_slimen_fit(mi355rec_slimen_t h, int32_t start_item, int32_t end_item, const uint32_t *seeds, double alpha, double l1_ratio,
                        int32_t positive, int32_t topK, int32_t max_iter, double tol);
/* Results of the last fit, per target t of its range: counts[t] kept coefficients in rows / values[t * slots_per_target ...] (unordered),
 * n_iter[t] sweeps run, converged[t] = 1 when the duality gap fell below tol * y.y.  slots_per_target = max(1, min(topK, n_items - 1)), n_items - 1 for topK = -1. */
int mi355rec_slimen_get(mi355rec_slimen_t h, int32_t *counts, int32_t *n_iter, int32_t *converged, int32_t *rows, float *values,
                        int32_t slots_per_target);
/* Rows [row0, row1) of G, row-major (row1 - row0) x n_items, into rows; diag (may be NULL) receives diag[row0:row1] (tests). */
int mi355rec_slimen_get_gram(mi355rec_slimen_t h, int32_t row0, int32_t row1, float *rows, float *diag);
int mi355rec_slimen_get_stats(mi355rec_slimen_t h, mi355rec_stats *stats);
/* Counters of the last fit: accepted coordinate changes (= rows of G streamed), sweeps, block steps (windows of draws), duality-gap
 * tests; h_in_lds = 1 when H was kept in LDS; gram_in_lds = 1 when the create call accumulated the rows of G in LDS; gram_ms = device
 * time of the Gram build of the create call. */
int mi355rec_slimen_fit_info(mi355rec_slimen_t h, int64_t *changes, int64_t *sweeps, int64_t *steps, int64_t *gap_tests,
                             int32_t *h_in_lds, int32_t *gram_in_lds, double *gram_ms);
void mi355rec_slimen_destroy(mi355rec_slimen_t h);

/* ------------------------------------------------------------------------------------------------------
 * PureSVD  (MatrixFactorization/PureSVDRecommender.py:34-47: sklearn's randomized_svd of URM_train) -- the device steps of the
 * randomized SVD; the loop and the r x r factorisations (Cholesky, eigh) run on the host
 * ---------------------------------------------------------------------------------------------------- */

typedef struct mi355rec_svd *mi355rec_svd_t;

/* URM_train (n_users x n_items) in both layouts, CSR and CSC, float32 values, indices inside the matrix; r = width of the two
 * resident blocks, side 0 (n_users x r) and side 1 (n_items x r), float32 row-major, zero after create.  r < 1, pointers that
 * decrease and indices outside the matrix are MI355REC_E_INVALID before the device is touched. */
int mi355rec_svd_create(mi355rec_svd_t *out, int32_t n_users, int32_t n_items, int32_t r, const int32_t *row_ptr, const int32_t *row_idx,
                        const float *row_val, const int32_t *col_ptr, const int32_t *col_idx, const float *col_val);
/* Upload / download of the block of a side (rows_of(side) x r floats). */
int mi355rec_svd_set_block(mi355rec_svd_t h, int32_t side, const float *X);
int mi355rec_svd_get_block(mi355rec_svd_t h, int32_t side, float *X);
/* dst_side 0: block[0] = URM . block[1];  dst_side 1: block[1] = URM^T . block[0].  Every output row is summed in a fixed order. */
int mi355rec_svd_product(mi355rec_svd_t h, int32_t dst_side);
/* G (r x r float64, row-major) = block[side]^T block[side], accumulated in float64. */
int mi355rec_svd_gram(mi355rec_svd_t h, int32_t side, double *G);
/* block[side] <- block[side] . T for T (r x r float32, row-major). */
int mi355rec_svd_apply(mi355rec_svd_t h, int32_t side, const float *T);
/* Timing of the last product (algorithmic_bytes = nnz (4 r + 8)). */
int mi355rec_svd_get_stats(mi355rec_svd_t h, mi355rec_stats *stats);
/* Totals since create: device milliseconds of the products, Gram builds and applies; kernel launches; calls of the entry points
 * above; bytes uploaded by create (the URM and its piece tables); host -> device and device -> host bytes since;
 * all_ones = 1 when the value stream is skipped. */
int mi355rec_svd_fit_info(mi355rec_svd_t h, double *product_ms, double *gram_ms, double *apply_ms, int64_t *launches, int64_t *calls,
                          int64_t *create_bytes, int64_t *h2d_bytes, int64_t *d2h_bytes, int32_t *all_ones);
void mi355rec_svd_destroy(mi355rec_svd_t h);

/* ------------------------------------------------------------------------------------------------------
 * NMF  (MatrixFactorization/NMFRecommender.py:58-71: sklearn.decomposition.NMF of URM_train, then its transform) -- the device steps of
 * the coordinate-descent and multiplicative-update solvers; the iteration loop, the permutations and the stop rule run on the host
 * 
 * ---------------------------------------------------------------------------------------------------- */

typedef struct mi355rec_nmf *mi355rec_nmf_t;

/* URM_train (n_users x n_items) in both layouts, CSR and CSC, float32 values >= 0, indices inside the matrix; k = number of
 * components.  Resident: side 0 = W (n_users x k) and side 1 = Ht = H^T (n_items x k), float32 row-major, zero after create, and one
 * value buffer of nnz floats per layout.  k outside [1, 4096], pointers that decrease, indices outside the matrix and negative
 * values are MI355REC_E_INVALID before the device is touched. */
int mi355rec_nmf_create(mi355rec_nmf_t *out, int32_t n_users, int32_t n_items, int32_t k, const int32_t *row_ptr, const int32_t *row_idx,
                        const float *row_val, const int32_t *col_ptr, const int32_t *col_idx, const float *col_val);
/* Upload / download of the block of a side (rows_of(side) x k floats); fill_block sets every cell to `value` (>= 0) on the device. */
int mi355rec_nmf_set_block(mi355rec_nmf_t h, int32_t side, const float *X);
int mi355rec_nmf_get_block(mi355rec_nmf_t h, int32_t side, float *X);
int mi355rec_nmf_fill_block(mi355rec_nmf_t h, int32_t side, float value);
/* One half-sweep of coordinate descent on block[side], the other block fixed (sklearn's _update_cdnmf_fast): for t in the order of
 * `permutation` (k entries, a permutation of 0 .. k-1, else MI355REC_E_INVALID) and every row i, grad = block[i] . G[t] - P[i][t],
 * block[i][t] = max(block[i][t] - grad / G[t][t], 0) where G[t][t] != 0; G = other^T other, P = URM . other (side 0) or URM^T . other
 * (side 1).  reuse = 1 keeps the G and P of the previous frobenius step on the same side (the other block has not changed; otherwise
 * MI355REC_E_INVALID).  The violation, sum of |projected gradient| in float64 in a fixed order, is added to a device total;
 * `violation` (nullable) receives that total and resets it, so the two half-sweeps of an iteration cost one 8-byte download. */
int mi355rec_nmf_cd_sweep(mi355rec_nmf_t h, int32_t side, const int32_t *permutation, int32_t reuse, double *violation);
/* One multiplicative update of block[side] (sklearn's _multiplicative_update_w / _h).  loss 0, frobenius: block *= P / (block . G), a
 * zero denominator replaced by float32 eps.  loss 1, Kullback-Leibler: q = x / max(W[i] . Ht[c], eps) per cell of the side's layout,
 * block *= (q-weighted product with the other block) / (column sums of the other block); a zero sum is float32 eps under W and 1
 * under Ht, and entries of Ht below float64 eps become 0.  reuse = 1 keeps G and P (frobenius) or the column sums (Kullback-Leibler)
 * of the previous step on the same side and loss.  Another loss is MI355REC_E_INVALID. */
int mi355rec_nmf_mu_step(mi355rec_nmf_t h, int32_t side, int32_t loss, int32_t reuse);
/* sklearn's _beta_divergence(X, W, H) in float64 sums of a fixed order.  loss 0: (|X|^2 + tr((W^T W)(H H^T)) - 2 sum (X H^T) o W) / 2;
 * loss 1: sum x log(x / max(wh, eps)) over the cells with x > eps + (sum W)(sum H) - sum x. */
int mi355rec_nmf_divergence(mi355rec_nmf_t h, int32_t loss, double *divergence);
/* Timing of the last fill_block / cd_sweep / mu_step / divergence call: call_ms = all its kernels, kernel_ms = its sweep, element-wise
 * pass or SDDMM. */
int mi355rec_nmf_get_stats(mi355rec_nmf_t h, mi355rec_stats *stats);
/* Totals since create.  phase_ms[6]: device milliseconds of the sparse products, the GEMMs, the sweeps, the element-wise passes,
 * the SDDMMs and the reductions (Gram, column sums, dot products, partial sums); kernel launches; calls of the entry points above;
 * bytes uploaded by create (the URM and its piece tables); host -> device and device -> host bytes since; all_ones = 1 when the URM
 * holds only ones. */
int mi355rec_nmf_fit_info(mi355rec_nmf_t h, double *phase_ms, int64_t *launches, int64_t *calls, int64_t *create_bytes, int64_t *h2d_bytes,
                          int64_t *d2h_bytes, int32_t *all_ones);
void mi355rec_nmf_destroy(mi355rec_nmf_t h);

/* ------------------------------------------------------------------------------------------------------
 * EASE_R  (EASE_R/EASE_R_Recommender.py:40-82: W = P / (-diag P) with P = (X^T X + diag)^-1, then similarityMatrixTopK) -- the Gram
 * matrix, its inverse, the weights and their column-wise top-K stay in HBM.  The device inverse is an
 * unpivoted blocked elimination: it serves symmetric POSITIVE-DEFINITE matrices and refuses every other one.
 * ---------------------------------------------------------------------------------------------------- */

typedef struct mi355rec_ease *mi355rec_ease_t;

/* An n_items x n_items float32 matrix on the device and the panel workspace of the elimination; MI355REC_E_INVALID, before anything
 * is launched, when they do not fit the device's free memory. */
int mi355rec_ease_create(mi355rec_ease_t *out, int32_t n_items);
/* The matrix <- X^T X of a similarity handle built with topK == 0 (shrink 0, normalize 0, cosine), on the device; the diagonal is 0.
 * A handle whose topK != 0 or whose n_cols != n_items is MI355REC_E_INVALID. */
int mi355rec_ease_set_gram_from_sim(mi355rec_ease_t h, mi355rec_sim_t sim);
/* Upload of any symmetric matrix (G[i * ld + j], host) / download of whatever the matrix currently holds. */
int mi355rec_ease_set_matrix(mi355rec_ease_t h, const float *G, int64_t ld);
int mi355rec_ease_get_matrix(mi355rec_ease_t h, float *G, int64_t ld);
/* The diagonal <- diag (n_items floats); needs a matrix that has been set and not yet inverted. */
int mi355rec_ease_set_diagonal(mi355rec_ease_t h, const float *diag);
/* The matrix <- its inverse, in place.  MI355REC_E_NUMERIC when a pivot is <= 0 or NaN -- the matrix is not positive definite;
 * mi355rec_last_error() names the step, the content of the matrix is then undefined and a new one has to be set. */
int mi355rec_ease_invert(mi355rec_ease_t h);
/* The same for any non-singular matrix, symmetric or not: blocked Gauss-Jordan elimination with partial (row) pivoting in float64 on
 * a float64 working copy (8 bytes per cell of the padded matrix, allocated at the first call and freed with the handle), the result
 * rounded to float32 into the matrix.  Preconditions and status as mi355rec_ease_invert; MI355REC_E_NUMERIC when a pivot is 0 or NaN
 * -- the matrix is singular; MI355REC_E_UNSUPPORTED, with the matrix untouched and nothing allocated, when the working copy does not
 * fit the device's free memory or is larger than MI355REC_EASE_PIVOT_MAX_BYTES (read at the first call of a handle). */
int mi355rec_ease_invert_pivoted(mi355rec_ease_t h);
/* Of the last mi355rec_ease_invert_pivoted: the swaps that moved a row, the smallest |pivot| of the pivot search, device milliseconds of
 * pivot search + row swaps and of the update GEMM.  MI355REC_E_INVALID when none has run on the matrix that is set. */
int mi355rec_ease_pivot_info(mi355rec_ease_t h, int32_t *moved_rows, double *min_pivot, double *pivot_ms, double *update_ms);
/* W[i * ld + j] = P[i][j] / -P[j][j], 0 on the diagonal (host, row-major).  Needs a successful invert, else MI355REC_E_INVALID. */
int mi355rec_ease_get_dense(mi355rec_ease_t h, float *W, int64_t ld);
/* Per column of W its topK largest NON-ZERO cells by value (similarityMatrixTopK, Base/Recommender_utils.py:55): idx / val
 * [n_items][topK], value-descending, ties towards the lower row, (-1, 0) padded.  topK > 4096 or columns beyond the in-LDS selection
 * (about 30 000 cells) are MI355REC_E_UNSUPPORTED. */
int mi355rec_ease_get_topk(mi355rec_ease_t h, int32_t topK, int32_t *idx, float *val);
/* Block size and number of steps of the elimination, the step that failed (-1: none), device milliseconds of the last invert, wall
 * milliseconds of the last set_gram_from_sim, device milliseconds of the weights (+ top-K) kernels, kernel launches since the last
 * invert. */
int mi355rec_ease_fit_info(mi355rec_ease_t h, int32_t *block, int32_t *steps, int32_t *failed_step, double *invert_ms, double *gram_ms,
                           double *topk_ms, int64_t *launches);
/* Of the last invert: algorithmic_flops = 2 n^3, algorithmic_bytes = 8 n^2 per step. */
int mi355rec_ease_get_stats(mi355rec_ease_t h, mi355rec_stats *stats);
void mi355rec_ease_destroy(mi355rec_ease_t h);

/* ------------------------------------------------------------------------------------------------------
 * Scoring + ranking of factor models  (Base/BaseMatrixFactorizationRecommender.py:38
 * _compute_item_score and the filter/rank half of Base/BaseRecommender.py:131 recommend)
 * ---------------------------------------------------------------------------------------------------- */

typedef struct mi355rec_scorer *mi355rec_scorer_t;

/* U (n_users x k), V (n_items x k) float32 row-major; biases only read when use_bias; the "seen" CSR is URM_train
 * (sorted or not), used by remove_seen. */
int mi355rec_scorer_create(mi355rec_scorer_t *out, int32_t n_users, int32_t n_items, int32_t n_factors,
                           const float *U, const float *V, int32_t use_bias, const float *user_bias, const float *item_bias,
                           float global_bias, const int32_t *seen_indptr, const int32_t *seen_indices);
/* New factor values of the same shapes (after more training epochs). */
int mi355rec_scorer_update(mi355rec_scorer_t h, const float *U, const float *V, const float *user_bias, const float *item_bias,
                           float global_bias);
/* The model of an MF training handle into the scorer, device to device.  Replaces mi355rec_mf_get_factors[_f64], the host's float64 ->
 * float32 pass and mi355rec_scorer_update: U, V (and, when the scorer has biases, user_bias, item_bias and global_bias) end bit for
 * bit as mi355rec_scorer_update leaves them for float32(what the getters return) -- the rows of the current parity buffers,
 * rounded to nearest.  n_users, n_items, n_factors and use_bias of the two handles must agree (MI355REC_E_INVALID, naming the
 * mismatch); an ASY_SVD handle is MI355REC_E_UNSUPPORTED (its user rows are item-sized, the user factors are estimated on the
 * host); a refused call leaves the scorer's model as it was.  The copy is queued behind the training handle's own work, after the
 * scorer's stream has drained, and has completed when the call returns.  get_stats of the scorer afterwards: call_ms = kernel_ms =
 * the copy kernels, algorithmic_bytes = bytes read + written. */
int mi355rec_scorer_update_from_mf(mi355rec_scorer_t scorer, mi355rec_mf_t mf);
/* The same from an IALS handle: replaces mi355rec_ials_get_factors, the host's float64 -> float32 pass and mi355rec_scorer_update.
 * U, V <- float32, rounded to nearest, of the two float64 matrices behind mi355rec_ials_device_factors; the scorer must have the
 * handle's n_users, n_items, n_factors and no biases. */
int mi355rec_scorer_update_from_ials(mi355rec_scorer_t scorer, mi355rec_ials_t ials);
/* For every user of the batch: scores = U[u] . V^T (+ biases); items with item_allowed[j] == 0 (nullable mask) and, when
 * remove_seen, the user's seen items become -inf; ranked[(row) * cutoff ...] = the cutoff best items in descending score
 * order, -1 padded where fewer finite scores exist.  scores (nullable, n x n_items) receives the filtered score matrix. */
int mi355rec_scorer_recommend(mi355rec_scorer_t h, const int32_t *user_ids, int32_t n, int32_t cutoff, int32_t remove_seen,
                              const uint8_t *item_allowed, int32_t *ranked, float *scores);
/* Candidate rows (the reference's EvaluatorNegativeItemSample, Base/Evaluation/Evaluator.py:455-539, hands each user's test items and
 * sampled negatives to recommend() as items_to_compute, Base/BaseRecommender.py:131-222): row r of the CSR (cand_indptr[n + 1],
 * cand_indices; item ids strictly ascending inside a row, else MI355REC_E_INVALID) holds the only items user_ids[r] may be given.
 * U[u] . V[c] (+ biases) is computed for those items alone -- no score matrix -- then the mask / seen filters of
 * mi355rec_scorer_recommend; ranked[(row) * cutoff ...] = the cutoff best candidates, descending, ties towards the lower item id,
 * -1 padded.  Rows of more than 4096 items and cutoffs above 4096 are MI355REC_E_UNSUPPORTED.  get_stats afterwards: kernel_ms =
 * call_ms = the candidate kernel(s) (there is no GEMM to tell apart), n_units = n; no flop or byte figures. */
int mi355rec_scorer_recommend_candidates(mi355rec_scorer_t h, const int32_t *user_ids, int32_t n, const int32_t *cand_indptr,
                                         const int32_t *cand_indices, int32_t cutoff, int32_t remove_seen, const uint8_t *item_allowed,
                                         int32_t *ranked);
/* Cells of the handle's n x n_items score buffer (0 until a full-row call has needed it): candidate calls leave it alone. */
int mi355rec_scorer_score_capacity(mi355rec_scorer_t h, int64_t *cells);
int mi355rec_scorer_get_stats(mi355rec_scorer_t h, mi355rec_stats *stats);
void mi355rec_scorer_destroy(mi355rec_scorer_t h);

/* Similarity models: scores[u] = A[u, :] . B, A (n_users x n_mid) and B (n_mid x n_items) CSR float32.
 * ItemKNN / SLIM: A = URM_train, B = W_sparse (Base/BaseSimilarityMatrixRecommender.py:73-92);
 * UserKNN: A = W_sparse, B = URM_train (:101-116).  Filtering and ranking as mi355rec_scorer_recommend. */
typedef struct mi355rec_spscorer *mi355rec_spscorer_t;
int mi355rec_spscorer_create(mi355rec_spscorer_t *out, int32_t n_users, int32_t n_mid, int32_t n_items,
                             const int32_t *a_indptr, const int32_t *a_indices, const float *a_data,
                             const int32_t *b_indptr, const int32_t *b_indices, const float *b_data,
                             const int32_t *seen_indptr, const int32_t *seen_indices);
int mi355rec_spscorer_recommend(mi355rec_spscorer_t h, const int32_t *user_ids, int32_t n, int32_t cutoff, int32_t remove_seen,
                                const uint8_t *item_allowed, int32_t *ranked, float *scores);
/* As mi355rec_scorer_recommend_candidates; the score row is accumulated as in mi355rec_spscorer_recommend and only the candidates
 * are read from it. */
int mi355rec_spscorer_recommend_candidates(mi355rec_spscorer_t h, const int32_t *user_ids, int32_t n, const int32_t *cand_indptr,
                                           const int32_t *cand_indices, int32_t cutoff, int32_t remove_seen,
                                           const uint8_t *item_allowed, int32_t *ranked);
/* The exact mode of the sparse scorer (off after create).  By default a score is a sum of float32 products whose order is decided by
 * which wavefront wins an LDS (or, for rows beyond 32 256 items, a global) float atomic: near-tied scores can change places between
 * two calls.  With exact != 0 every score is SciPy's csr @ csr bit for bit: from +0.0f, over the stored cells (m, w) of the user's row
 * of A IN STORAGE ORDER (A's indices are used as given, never sorted) and, for each, over the stored cells (j, b) of row m of B,
 * s[j] = s[j] + (w * b) in float32 with the product rounded before the add.  No float atomic runs; the same call gives the same bytes
 * every time, however a batch is cut into blocks; a candidate's score is the cell of the full row.  It applies to
 * mi355rec_spscorer_recommend[_candidates] and to mi355rec_eval_add_spscorer[_candidates] alike.
 * Switching it on runs one device pass over B: every row must hold its column ids strictly ascending inside [0, n_items) (sort B's
 * indices first; a column stored twice in a row cannot be served).  Otherwise MI355REC_E_INVALID, the message names the first
 * offending row, the mode is unchanged and the handle stays usable.  exact == 0 switches back to the atomic kernels.
 * get_stats after an exact recommend: kernel_ms = call_ms = the exact scoring kernel (recommend_candidates: that kernel and the
 * candidates' gather + ranking). */
int mi355rec_spscorer_set_exact(mi355rec_spscorer_t h, int32_t exact);
/* Replaces B by another host CSR of the same n_mid x n_items, with any number of cells; A and the seen CSR stay where they are.
 * Afterwards the scorer answers mi355rec_spscorer_recommend[_candidates] and mi355rec_eval_add_spscorer[_candidates] exactly as one
 * freshly created with that B would, in either mode; in exact mode the table of the mode is rebuilt for the new B.
 * MI355REC_E_INVALID, checked on the host before anything is uploaded, the message naming the first offending row: a NULL argument,
 * row pointers that do not start at 0 or that decrease, a column id outside [0, n_items) and -- in exact mode -- a row whose ids are
 * not strictly ascending.  A refused call leaves the scorer's B and mode as they were and the handle usable: the new B is written
 * into spare buffers and swapped in once it has been accepted.  The scorer's stream is drained first (an evaluator may still have
 * lists queued that read the old B).  get_stats: call_ms = kernel_ms = the copies (and the exact pass), algorithmic_bytes = what
 * they read and wrote on the device. */
int mi355rec_spscorer_update_b(mi355rec_spscorer_t h, const int32_t *b_indptr, const int32_t *b_indices, const float *b_data);
/* Downloads B as the scorer holds it: indptr[n_mid + 1], and *nnz entries of indices and data.  With indices == NULL (and
 * data == NULL) only indptr and *nnz come back: call once for the size, then again with arrays of that size. */
int mi355rec_spscorer_get_b(mi355rec_spscorer_t h, int32_t *indptr, int32_t *indices, float *data, int64_t *nnz);
/* B <- the CSR that mi355rec_slim_get_W_csr(slim, topK, ...) would return -- indptr, indices and data bit for bit -- device to
 * device: it replaces that download, the host's assembly of the matrix and the creation of a new scorer with A, the seen CSR and W
 * uploaded again.  The SLIM handle is only read.  Ordering: the scorer's stream is drained; the build of W and the copy are queued
 * on the SLIM handle's stream behind its own work; the call returns after that stream has been waited for.  Refusals, which leave
 * the scorer as it was: MI355REC_E_INVALID for a NULL handle, for a SLIM handle whose n_items is not both n_mid and n_items of the
 * scorer (a user-based scorer; the message names the values) and for topK < 1; MI355REC_E_UNSUPPORTED for a handle created with
 * train_with_sparse_weights (reading its model prunes it), for n_items > 65 535 and for a topK beyond the in-LDS selection, as
 * mi355rec_slim_get_W_csr.  In exact mode the table is rebuilt.  get_stats of the scorer: call_ms = kernel_ms = the device work of
 * the call, algorithmic_bytes = the weight store read once + W read and written (+ the exact pass). */
int mi355rec_spscorer_update_from_slim(mi355rec_spscorer_t h, mi355rec_slim_t slim, int32_t topK);
int mi355rec_spscorer_get_stats(mi355rec_spscorer_t h, mi355rec_stats *stats);
void mi355rec_spscorer_destroy(mi355rec_spscorer_t h);

/* Similarity models whose weights are a DENSE array: scores[u] = A[u, :] . B, A (n_users x n_mid) CSR float32, B (n_mid x n_items)
 * float32 row-major -- Base/BaseSimilarityMatrixRecommender.py:73-92 with a W_sparse that is an ndarray, what
 * EASE_R_Recommender.fit(topK=None) leaves (EASE_R/EASE_R_Recommender.py:40-82).  Every score is SciPy's csr @ ndarray bit for bit:
 * from +0.0f, over the row's stored cells IN STORAGE ORDER (the indices are used as given, never sorted), acc = acc + (a * B[i][j])
 * in float32 with the product rounded before the add.  The same call gives the same bytes every time.  B is not checked for
 * non-finite values: they are scored as IEEE arithmetic gives them, and a NaN score is never listed.  Filtering and ranking as
 * mi355rec_scorer_recommend.
 * create: B (nullable: zero weights until update / set_from_ease) is copied to the device; MI355REC_E_INVALID, before anything is
 * allocated or launched, when it does not fit the device's free memory, and for column ids outside their range. */
typedef struct mi355rec_dscorer *mi355rec_dscorer_t;
int mi355rec_dscorer_create(mi355rec_dscorer_t *out, int32_t n_users, int32_t n_mid, int32_t n_items, const int32_t *a_indptr,
                            const int32_t *a_indices, const float *a_data, const float *B, const int32_t *seen_indptr,
                            const int32_t *seen_indices);
/* A new B of the same shape; nothing is reallocated. */
int mi355rec_dscorer_update(mi355rec_dscorer_t h, const float *B);
/* B <- the weights of an EASE handle after a successful invert (the cells mi355rec_ease_get_dense downloads), device to device.
 * The scorer must be n_items x n_items for the handle's n_items.  get_stats afterwards: call_ms = kernel_ms = the copy. */
int mi355rec_dscorer_set_from_ease(mi355rec_dscorer_t h, mi355rec_ease_t ease);
/* get_stats afterwards: kernel_ms = the scoring kernel, call_ms = scoring + ranking, algorithmic_bytes = 4 * n_items * (stored cells of
 * the batch's rows of A): every stored cell streams one row of B. */
int mi355rec_dscorer_recommend(mi355rec_dscorer_t h, const int32_t *user_ids, int32_t n, int32_t cutoff, int32_t remove_seen,
                               const uint8_t *item_allowed, int32_t *ranked, float *scores);
/* As mi355rec_scorer_recommend_candidates; a candidate's score is bitwise the cell of the full row. */
int mi355rec_dscorer_recommend_candidates(mi355rec_dscorer_t h, const int32_t *user_ids, int32_t n, const int32_t *cand_indptr,
                                          const int32_t *cand_indices, int32_t cutoff, int32_t remove_seen,
                                          const uint8_t *item_allowed, int32_t *ranked);
int mi355rec_dscorer_get_stats(mi355rec_dscorer_t h, mi355rec_stats *stats);
void mi355rec_dscorer_destroy(mi355rec_dscorer_t h);

/* ------------------------------------------------------------------------------------------------------
 * Non-personalized models: one vector of item scores for every user  (Base/NonPersonalizedRecommender.py:30-43,119-132
 * _compute_item_score of TopPop / GlobalEffects repeats it per user; Base/BaseRecommender.py:131-222 recommend filters and ranks)
 * ---------------------------------------------------------------------------------------------------- */

typedef struct mi355rec_itemscorer *mi355rec_itemscorer_t;

/* item_scores: float32[n_items]; the "seen" CSR is URM_train (rows sorted or not, repeats allowed).  The vector is sorted once, here
 * and in update: a user's list is the head of that order without the user's seen items -- work of cutoff + profile length per user. */
int mi355rec_itemscorer_create(mi355rec_itemscorer_t *out, int32_t n_users, int32_t n_items, const float *item_scores,
                               const int32_t *seen_indptr, const int32_t *seen_indices);
/* The same with the seen CSR in device memory (a resident URM's indptr / indices, seen_nnz cells): copied device to device. */
int mi355rec_itemscorer_create_resident(mi355rec_itemscorer_t *out, int32_t n_users, int32_t n_items, const float *item_scores,
                                        const int32_t *d_seen_indptr, const int32_t *d_seen_indices, int64_t seen_nnz);
/* A new vector of the same length. */
int mi355rec_itemscorer_update(mi355rec_itemscorer_t h, const float *item_scores);
/* As mi355rec_scorer_recommend: ranked[(row) * cutoff ...] = the cutoff best items that are finite in the vector, allowed by the
 * mask (nullable) and -- remove_seen -- not seen by the user; score descending, ties towards the lower item id, -1 padded.  A
 * non-finite entry of the vector is never listed.  scores (nullable, n x n_items): the vector in every row, -inf where a filter
 * applies. */
int mi355rec_itemscorer_recommend(mi355rec_itemscorer_t h, const int32_t *user_ids, int32_t n, int32_t cutoff, int32_t remove_seen,
                                  const uint8_t *item_allowed, int32_t *ranked, float *scores);
/* As mi355rec_scorer_recommend_candidates: the vector is gathered at the candidates of each row. */
int mi355rec_itemscorer_recommend_candidates(mi355rec_itemscorer_t h, const int32_t *user_ids, int32_t n, const int32_t *cand_indptr,
                                             const int32_t *cand_indices, int32_t cutoff, int32_t remove_seen,
                                             const uint8_t *item_allowed, int32_t *ranked);
/* W: positions of the order one pass of the ranking kernel covers -- 2048 with a wavefront per user, 8192 with a 256-lane
 * workgroup per user.  set_window_bits chooses between the two kernel shapes (any other value is MI355REC_E_INVALID). */
int mi355rec_itemscorer_window_bits(mi355rec_itemscorer_t h, int32_t *bits);
int mi355rec_itemscorer_set_window_bits(mi355rec_itemscorer_t h, int32_t bits);
/* kernel_ms = call_ms = everything the last recommend / recommend_candidates put on the stream; n_units = n. */
int mi355rec_itemscorer_get_stats(mi355rec_itemscorer_t h, mi355rec_stats *stats);
void mi355rec_itemscorer_destroy(mi355rec_itemscorer_t h);

/* TopPop.fit (Base/NonPersonalizedRecommender.py:23-27): item_counts[n_items] = stored cells per column of the CSR matrix, without
 * a CSC copy.  _resident: the arrays are device pointers (nnz stored cells); item_counts is host memory in both. */
int mi355rec_urm_item_counts(int32_t n_users, int32_t n_items, const int32_t *indptr, const int32_t *indices, int32_t *item_counts);
int mi355rec_urm_item_counts_resident(int32_t n_users, int32_t n_items, int32_t nnz, const int32_t *d_indptr, const int32_t *d_indices,
                                      int32_t *item_counts);
/* GlobalEffects.fit (:71-116) on the CSR matrix: mu = float32(sum x / nnz); d = float32(x - mu); item_bias[c] = sum over column c of
 * d / (col_nnz + lambda_item); d' = float32(double(d) - item_bias[col]); user_bias[r] = sum over row r of d' / (row_nnz +
 * lambda_user).  Sums are float64 in a fixed order (the same bits on every run); the outputs are host memory. */
int mi355rec_urm_global_effects(int32_t n_users, int32_t n_items, const int32_t *indptr, const int32_t *indices, const float *data,
                                double lambda_user, double lambda_item, float *mu, double *item_bias, double *user_bias);
int mi355rec_urm_global_effects_resident(int32_t n_users, int32_t n_items, int32_t nnz, const int32_t *d_indptr, const int32_t *d_indices,
                                         const float *d_data, double lambda_user, double lambda_item, float *mu, double *item_bias,
                                         double *user_bias);

/* ------------------------------------------------------------------------------------------------------
 * Holdout evaluation  (Base/Evaluation/Evaluator.py:225-275 evaluateRecommender, :294-374 _compute_metrics_on_recommendation_list,
 * :404-450 EvaluatorHoldout._run_evaluation_on_selected_users; the metric functions of Base/Evaluation/metrics.py)
 * ---------------------------------------------------------------------------------------------------- */

typedef struct mi355rec_eval *mi355rec_eval_t;

/* Per-user values of every cutoff, in this order (fp64; the float32 metrics hold their exact float32 value):
 * roc_auc (metrics.py:102-118), precision (:136-144), precision_recall_min_denominator (:147-155), recall (:159-164),
 * average_precision (:65-74), rr (:167-175), ndcg (:180-209), hits (Evaluator.py:339 HIT_RATE), arhr (:122-133), the Novelty sum
 * (:562-572), the AveragePopularity mean (:614-621), and 1 when the list is not empty (Coverage_User, :361-362). */
#define MI355REC_EVAL_VALUES 12

/* URM_test AS PASSED (Evaluator.py:171, 279-291) as CSR with its stored values (the relevance of ndcg); rows need not be sorted.
 * Lists are min(max(cutoffs), n_items) wide; the ideal DCG of every user (all of its test ratings, metrics.py:194) is computed
 * here.  log_table = np.log(np.arange(log_len, dtype=np.float32) + 2) (metrics.py:208), log_len >= max(list width, longest
 * test row).  Cutoffs must be distinct. */
int mi355rec_eval_create(mi355rec_eval_t *out, int32_t n_users, int32_t n_items, const int32_t *test_indptr,
                         const int32_t *test_indices, const double *test_relevance, const int32_t *cutoffs, int32_t n_cutoffs,
                         const float *log_table, int32_t log_len);
/* Starts an evaluation: per-item Novelty terms -log2(pop / n_interactions) / n_items (0 where pop == 0) and AveragePopularity terms
 * pop / max(pop) (metrics.py:552-559, 601-611; pop = column counts of the recommender's URM_train), and the user ids of the whole
 * evaluation, uploaded once.  Zeroes the accumulators. */
int mi355rec_eval_begin(mi355rec_eval_t h, const double *novelty_term, const double *popularity_term, const int32_t *user_ids,
                        int32_t n_eval);
/* Evaluation positions [first, first + n): ranked[(row) * width ...] host lists, -1 padded at the end (Evaluator.py:436-442). */
int mi355rec_eval_add_lists(mi355rec_eval_t h, int32_t first, int32_t n, const int32_t *ranked);
/* The same users scored and ranked by a device scorer (as mi355rec_scorer_recommend / mi355rec_spscorer_recommend with
 * cutoff = the list width); the lists never leave the device.  Asynchronous: the metric kernel runs on the scorer's stream. */
int mi355rec_eval_add_scorer(mi355rec_eval_t h, mi355rec_scorer_t scorer, int32_t first, int32_t n, int32_t remove_seen,
                             const uint8_t *item_allowed);
int mi355rec_eval_add_spscorer(mi355rec_eval_t h, mi355rec_spscorer_t scorer, int32_t first, int32_t n, int32_t remove_seen,
                               const uint8_t *item_allowed);
int mi355rec_eval_add_itemscorer(mi355rec_eval_t h, mi355rec_itemscorer_t scorer, int32_t first, int32_t n, int32_t remove_seen,
                                 const uint8_t *item_allowed);
int mi355rec_eval_add_dscorer(mi355rec_eval_t h, mi355rec_dscorer_t scorer, int32_t first, int32_t n, int32_t remove_seen,
                              const uint8_t *item_allowed);
/* Negative-sample evaluation (Evaluator.py:455-539 EvaluatorNegativeItemSample): the candidate rows of ALL n_users users as CSR
 * (indptr[n_users + 1]; item ids strictly ascending inside a row, else MI355REC_E_INVALID), uploaded once per evaluator.
 * MI355REC_E_UNSUPPORTED when a row holds more than 4096 items or the lists are more than 4096 wide. */
int mi355rec_eval_set_candidates(mi355rec_eval_t h, const int32_t *indptr, const int32_t *indices);
/* mi355rec_eval_add_scorer / mi355rec_eval_add_spscorer with every user ranking the candidates of its row only (as
 * mi355rec_*scorer_recommend_candidates).  The two functions above are not affected by mi355rec_eval_set_candidates. */
int mi355rec_eval_add_scorer_candidates(mi355rec_eval_t h, mi355rec_scorer_t scorer, int32_t first, int32_t n, int32_t remove_seen,
                                        const uint8_t *item_allowed);
int mi355rec_eval_add_spscorer_candidates(mi355rec_eval_t h, mi355rec_spscorer_t scorer, int32_t first, int32_t n, int32_t remove_seen,
                                          const uint8_t *item_allowed);
int mi355rec_eval_add_itemscorer_candidates(mi355rec_eval_t h, mi355rec_itemscorer_t scorer, int32_t first, int32_t n, int32_t remove_seen,
                                            const uint8_t *item_allowed);
int mi355rec_eval_add_dscorer_candidates(mi355rec_eval_t h, mi355rec_dscorer_t scorer, int32_t first, int32_t n, int32_t remove_seen,
                                         const uint8_t *item_allowed);
/* sums[c * MI355REC_EVAL_VALUES + v]: value v summed over the evaluated users in a fixed order (the last one is the covered-user
 * count); item_counts[c * n_items + i]: times item i was recommended within cutoff c (the recommended_counter of
 * metrics.py:284-286, 762-769). */
int mi355rec_eval_finish(mi355rec_eval_t h, double *sums, int32_t *item_counts);
/* out[(p * n_cutoffs + c) * MI355REC_EVAL_VALUES + v]: the per-user values of the last evaluation, p = position of the user. */
int mi355rec_eval_get_per_user(mi355rec_eval_t h, double *out);
/* DIVERSITY_SIMILARITY (metrics.py:641-694 Diversity_similarity, Evaluator.py:353-354).  matrix: the dense item diversity matrix,
 * n_items x n_items cells of elem_bytes (4: float32, 8: float64), row-major, host memory; indexed [row = items[i], column = items[j]]
 * and not assumed symmetric.  Waits for the blocks under way, uploads the cells and checks on the device that every one lies in
 * [0, 1] (MI355REC_E_INVALID otherwise, NaN included; the matrix is then not kept).  MI355REC_E_UNSUPPORTED when the lists are more
 * than 1024 wide.  matrix == NULL takes the matrix away.  Either way the change holds from the next mi355rec_eval_begin on: with a
 * matrix set, begin zeroes a buffer of [n_eval][n_cutoffs] float64 values of its own, every add_* call fills the rows of its users
 * (for one user and cutoff, with `items` the first L = min(cutoff, list length) entries:
 *     sum over i = 0 .. L-2, j = 0 .. L-1, j != i of matrix[items[i]][items[j]], divided by L (L - 1);
 * NaN where L < 2, the reference divides by zero there), and finish sums them in a fixed order.  MI355REC_EVAL_VALUES, the layout of
 * mi355rec_eval_finish's sums and of mi355rec_eval_get_per_user are not affected. */
int mi355rec_eval_set_diversity(mi355rec_eval_t h, const void *matrix, int32_t elem_bytes);
/* After mi355rec_eval_finish of an evaluation begun with a matrix set: sums[c] over the evaluated users, cutoffs in the given order;
 * per_user (NULL, or [n_eval][n_cutoffs]) the values themselves. */
int mi355rec_eval_get_diversity(mi355rec_eval_t h, double *sums, double *per_user);
/* elem_bytes of the matrix that is set (0: none) and the host time of the last mi355rec_eval_set_diversity: allocation + upload, and
 * the range check with its read-back. */
int mi355rec_eval_diversity_info(mi355rec_eval_t h, int32_t *elem_bytes, double *upload_ms, double *check_ms);
void mi355rec_eval_destroy(mi355rec_eval_t h);

#ifdef __cplusplus
}
#endif
#endif /* MI355REC_H */
