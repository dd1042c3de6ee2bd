/*
 * bicgstab_hip.h -- C ABI of libbicgstab_hip.so: the MI355X (gfx950) BiCGStab hot path.
 *
 * Drop-in boundary: the four solver entry points of the reference's solver.h, byte-for-byte the
 * same signatures and struct layouts, so that the reference's C host (main.c + matrix.c + mmio.c)
 * links against this library instead of its own solver.c / vector.c.
 * Everything else in this header is additive (handle-based API for callers that keep the matrix
 * resident on the GPU, kernel-level entry points for parity tests and benchmarks, communicator
 * bootstrap). Plain C types only.
 *
 * All arithmetic is fp64, all indices uint32, exactly as in the reference (src/matrix.h:19-26).
 */
#ifndef BICGSTAB_HIP_H
#define BICGSTAB_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Matrix containers. If the reference's matrix.h was included first (its include guard is
 * MATRIX_H) its own typedefs are used; otherwise layout-identical ones are declared here.
 *   CSR_Matrix  <- reference src/matrix.h:19-26   (sizeof 40)
 *   INFO_Matrix <- reference src/matrix.h:28-33   (sizeof 32; MM_typecode = char[4], mmio.h:16)
 * Per rank: diag = rows x rows block with LOCAL column indices, offd = rows x n block with
 * GLOBAL column indices (reference src/matrix.c:343-351, 380-392); displs[p]/recvcounts[p] =
 * first row / row count of rank p (src/matrix.c:306-307).
 * ------------------------------------------------------------------------------------------- */
#ifndef MATRIX_H
typedef struct {
    double       *val;
    unsigned int *col;
    unsigned int *ptr;
    unsigned int  nz;
    unsigned int  rows;
    unsigned int  cols;
} CSR_Matrix;

typedef struct {
    unsigned int nz, rows, cols;
    char         code[4];
    int         *recvcounts;
    int         *displs;
} INFO_Matrix;
#endif

/* ---------------------------------------------------------------------------------------------
 * 1. Drop-in entry points (replace reference src/solver.c).
 *
 *   bicgstab          <- src/solver.h:10 (implementation src/solver.c:35-146)
 *   ca_bicgstab       <- src/solver.h:11 (src/solver.c:160-278)
 *   pipe_bicgstab     <- src/solver.h:12 (src/solver.c:292-417)
 *   pipe_bicgstab_rr  <- src/solver.h:13 (src/solver.c:433-576)
 *
 * Semantics kept: collective over all ranks; x_loc in = x0, out = solution; r_loc in = b,
 * out = recursive residual (src/solver.c:75); return value = iterations executed; non-square
 * matrix prints "Error: matrix is not square." and exit(1) (src/solver.c:43-46); rank 0 prints
 * the reference's progress and summary lines verbatim (src/solver.c:124,135-139). The matrix is
 * never modified. Constants default to the reference's (EPS 1e-15, MAX_ITER 1000, OUT_ITER 100;
 * src/solver.c:3-9) and can be overridden without an ABI change through the environment:
 * BICG_TOL, BICG_MAX_ITER, BICG_OUT_ITER, BICG_CHECK_EVERY, BICG_QUIET, BICG_RR_DRIFT (adaptive
 * residual replacement for the pipelined solvers, off by default).
 *
 * Rank discovery: if the process has initialised MPI (the reference's main.c does) the library
 * picks rank/size up from MPI_COMM_WORLD through weak symbols and bootstraps RCCL with an
 * MPI_Bcast of the unique id; otherwise it runs single-rank unless a bicg_comm_init_* call was
 * made first. HIP / RCCL failures print to stderr and exit(EXIT_FAILURE).
 * ------------------------------------------------------------------------------------------- */
int bicgstab(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc, double *r_loc);
int ca_bicgstab(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc, double *r_loc);
int pipe_bicgstab(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc, double *r_loc);
int pipe_bicgstab_rr(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc, double *r_loc, int krr, int nrr);
/* Not in the reference: bicgstab() right-preconditioned with M = diag(A) (Jacobi; BICG_BICGSTAB_DIAG, section 3). Same signature,
 * semantics and printed lines as bicgstab(); r_loc comes back as the recursive residual of A x = b itself, and the stopping test
 * is bicgstab()'s. The diagonal is read from A_loc_diag (bicg_csr_diagonal, section 5) and installed on the resident drop-in
 * context by every call -- created, refreshed or reused, and whatever diagonal was installed on it in between. A block in which some row stores no (i,i) entry prints
 * "Error: matrix has rows without a diagonal entry." to stderr and exit(1); a stored zero is refused the same way. */
int jacobi_bicgstab(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc, double *r_loc);
/* Not in the reference: bicgstab() right-preconditioned with the bs x bs diagonal blocks of A (block Jacobi; BICG_BICGSTAB_BLOCK,
 * section 3), bs = 1..16: the unknowns per node of the caller's numbering. Semantics and printed lines are bicgstab()'s. The blocks
 * are read from A_loc_diag (bicg_csr_block_diagonal, section 5; they never cross a rank's boundary) and installed on the resident
 * drop-in context by every call. A block that cannot be inverted prints "Error: matrix has a singular diagonal block." to stderr
 * and exit(1); a bs outside 1..16 prints "Error: block size <bs> is outside 1..16." and exit(1). */
int block_jacobi_bicgstab(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc, double *r_loc, int bs);
/* Not in the reference: BiCGStab(2) (BICG_BICGSTAB2, section 3), for matrices on which bicgstab() stagnates or breaks down -- strong
 * convection, eigenvalues with large imaginary parts. bicgstab()'s arguments, printed lines, environment overrides and resident
 * context; the return value and the progress lines count BiCG steps (two products each, bicgstab()'s unit), two per sweep. */
int bicgstab2(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc, double *r_loc);
/* Not in the reference: bicgstab2() right-preconditioned with M = diag(A) (BICG_BICGSTAB2_DIAG) or with the bs x bs diagonal blocks
 * of A (BICG_BICGSTAB2_BLOCK; section 3), for matrices that are convective and badly scaled or block-coupled. Arguments, printed lines
 * and counting are bicgstab2()'s; the preconditioner is read from A_loc_diag and installed by every call, and the error lines and
 * exits are those of jacobi_bicgstab() / block_jacobi_bicgstab(). */
int jacobi_bicgstab2(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc, double *r_loc);
int block_jacobi_bicgstab2(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc, double *r_loc, int bs);

/* Shifted systems (A + sigma_j I) x_j = b, j = 0..sigma_len-1, solved with ONE Krylov recurrence on
 * the seed system (2 SpMV per iteration whatever the number of shifts) -- all six entry points of
 * reference src/shifted_solver.h:16-21:
 *
 *   shifted_bicgstab                    <- :16 (src/shifted_solver.c:13-180)   seed = A, xi/tau recurrences
 *   shifted_lopbicgstab                 <- :17 (:182-354)   seed = A + sigma[seed] I
 *   shifted_lopbicgstab_v2              <- :18 (:357-529)   same arithmetic as :17, re-ordered
 *   shifted_lopbicgstab_nooverlap       <- :19 (:531-701)   same arithmetic as :17, re-ordered
 *   shifted_pipe_lopbicgstab            <- :20 (:703-895)   pipelined recurrence
 *   shifted_pipe_lopbicgstab_nooverlap  <- :21 (:897-1086)  same arithmetic as :20, re-ordered
 *
 * (the re-ordered reference functions are bit-identical to their base function; each group resolves
 * to one implementation here). x_loc_set is shift-major, x_loc_set[j * local_rows + i]
 * (src/shifted_solver.c:118-123), in = initial guess (the reference's drivers pass 0), out = the
 * sigma_len solutions; r_loc in = b, out = seed residual. Convergence: max_j |1/(zeta_j pi_j)|^2 (r,r)
 * <= EPS^2 (b,b) (xi/tau form: max_j |xi_j tau_j|), EPS 1e-12, MAX_ITER 1000 (src/shifted_solver.c:5-6). */
int shifted_bicgstab(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc_set, double *r_loc, double *sigma, int sigma_len);
int shifted_lopbicgstab(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc_set, double *r_loc, double *sigma, int sigma_len, int seed);
int shifted_lopbicgstab_v2(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc_set, double *r_loc, double *sigma, int sigma_len, int seed);
int shifted_lopbicgstab_nooverlap(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc_set, double *r_loc, double *sigma, int sigma_len, int seed);
int shifted_pipe_lopbicgstab(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc_set, double *r_loc, double *sigma, int sigma_len, int seed);
int shifted_pipe_lopbicgstab_nooverlap(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc_set, double *r_loc, double *sigma, int sigma_len, int seed);
/* Shifted solvers with per-shift convergence flags and SEED SWITCHING, reference
 * src/shifted_switching_solver.h:10-12:
 *   shifted_lopbicg                   <- :10 (src/shifted_switching_solver.c:20-257)   a shift whose residual bound
 *                                        |1/(zeta pi)| ||r|| has reached EPS is frozen; ends when all have converged
 *   shifted_lopbicg_switching         <- :11 (:260-608)   as above; when the seed converges first, the slowest
 *                                        remaining shift becomes the seed (history of alpha/beta/omega/pi re-derived)
 *   shifted_lopbicg_switching_noovlp  <- :12 (:611-1016)  same arithmetic, different MPI_Wait placement
 * Same arguments as shifted_lopbicgstab. r_loc returns the (rescaled) residual of the final seed. Return value as
 * in the reference: iterations for shifted_lopbicg, iterations + 1 for the switching variants (k starts at 1). */
int shifted_lopbicg(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc_set, double *r_loc, double *sigma, int sigma_len, int seed);
int shifted_lopbicg_switching(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc_set, double *r_loc, double *sigma, int sigma_len, int seed);
int shifted_lopbicg_switching_noovlp(CSR_Matrix *A_loc_diag, CSR_Matrix *A_loc_offd, INFO_Matrix *A_info, double *x_loc_set, double *r_loc, double *sigma, int sigma_len, int seed);

/* ---------------------------------------------------------------------------------------------
 * 2. Communicator bootstrap (process-global; one process per GPU).
 *    The reference uses MPI_COMM_WORLD implicitly (src/solver.c:37, src/matrix.c:432); here the
 *    transport is explicit: RCCL over xGMI for production, or a host-staged transport driven by
 *    caller-supplied callbacks (MPI, gloo, ...) for tests and for more ranks than GPUs.
 * ------------------------------------------------------------------------------------------- */
#define BICG_UNIQUE_ID_BYTES 128

/* rank 0: create an RCCL unique id to broadcast to the other ranks by any means */
int bicg_comm_unique_id(void *id_out /* BICG_UNIQUE_ID_BYTES */);
/* all ranks: join. device = HIP device ordinal for this process (-1: rank % device count). Returns 0; with
 * BICG_COMM_SOFT_FAIL=1 in the environment a failing ncclCommInitRank returns 1 instead of exiting (no
 * communicator is installed then -- the caller picks another transport on all ranks). */
int bicg_comm_init_rccl(int rank, int nranks, const void *id, int device);

/* Host-staged transport. Callbacks operate on HOST buffers and are collective.
 *   allreduce_sum: in-place sum of n doubles over all ranks (replaces MPI_Iallreduce+MPI_Wait of
 *                  one double each, e.g. reference src/solver.c:90-91, here packed)
 *   alltoallv:     byte-wise personalised exchange (counts/displs in BYTES, per peer), replaces
 *                  the full-vector MPI_Iallgatherv of reference src/matrix.c:432 with a halo */
typedef void (*bicg_allreduce_fn)(double *buf, int n, void *user);
typedef void (*bicg_alltoallv_fn)(const void *send, const int *scounts, const int *sdispls,
                                  void *recv, const int *rcounts, const int *rdispls, void *user);
int bicg_comm_init_host(int rank, int nranks, bicg_allreduce_fn allreduce, bicg_alltoallv_fn alltoallv,
                        void *user, int device);
/* MPI_COMM_WORLD of the calling process through weak symbols; transport "rccl" or "host".
 * Returns non-zero when the process has no initialised MPI. */
int bicg_comm_init_mpi(const char *transport, int device);
int bicg_comm_init_single(int device);
/* Collective, after one of the init calls above: switch the DATA path (halo values, dot sums) to direct
 * peer-to-peer stores between the GPUs of one node -- mailboxes mapped through HIP IPC, written by the
 * producing kernels, no library collective per exchange (the replacement for the MPI_Iallgatherv /
 * MPI_Iallreduce pair of reference src/matrix.c:432, src/solver.c:90 that a 20 us iteration can afford).
 * Ends with a self-test over the real links; returns 0 when it passed on EVERY rank, otherwise nothing
 * changes and the transport's own collectives stay in use. bicg_comm_init_mpi("auto") tries it itself.
 * BICG_P2P=0 disables it. */
int bicg_comm_enable_p2p(void);
/* 0: not active; 1: active, mailboxes in ordinary device memory; 2: active, uncached device memory */
int bicg_comm_p2p_active(void);
void bicg_comm_finalize(void);
/* 1 when librccl and every entry point the RCCL transport uses resolve (dies with a message otherwise); no device call */
int bicg_comm_rccl_loadable(void);
/* Why the last bicg_comm_init_rccl of this process failed: RCCL's result string and, where the library has it, its own last
 * error text ("" after a success). Returns the text's length. With BICG_COMM_SOFT_FAIL=1 a refused communicator is reported
 * this way instead of ending the process (bench.py records RCCL's refusal of two ranks on one device verbatim). */
int bicg_comm_last_error(char *out, int cap);
/* one-rank RCCL round trip (library load, communicator, all-reduce); 0 = ok. Needs a GPU. */
int bicg_comm_selftest_rccl(int device);
int bicg_comm_rank(void);
int bicg_comm_size(void);

/* ---------------------------------------------------------------------------------------------
 * 3. Handle-based API: upload once, solve many times, vectors may stay resident in HBM.
 * ------------------------------------------------------------------------------------------- */
typedef struct bicg_ctx bicg_ctx;

enum { BICG_BICGSTAB = 0, BICG_CA_BICGSTAB = 1, BICG_PIPE_BICGSTAB = 2, BICG_PIPE_BICGSTAB_RR = 3,
       BICG_BICGSTAB_DIAG = 4,  /* BICG_BICGSTAB right-preconditioned with the diagonal of bicg_precond_diagonal (below) */
       BICG_BICGSTAB_BLOCK = 5, /* BICG_BICGSTAB right-preconditioned with the block diagonal of bicg_precond_block_diagonal (below) */
       BICG_BICGSTAB2 = 6,      /* BiCGStab(2): two BiCG steps and a two-dimensional minimal-residual step per sweep (below) */
       BICG_BICGSTAB2_DIAG = 7, /* BICG_BICGSTAB2 right-preconditioned with the diagonal of bicg_precond_diagonal (below) */
       BICG_BICGSTAB2_BLOCK = 8 /* BICG_BICGSTAB2 right-preconditioned with the block diagonal of bicg_precond_block_diagonal (below) */ };

/* BICG_BICGSTAB2 -- Sleijpen-Fokkema BiCGStab(l) with l = 2. BICG_BICGSTAB's stabilising step minimises the
 * residual over ONE direction and degenerates (omega -> 0) when A has eigenvalues with large imaginary parts, which is what a
 * convection term does; this method minimises over two, by the 2 x 2 normal equations. r# is the shadow residual, r0 the residual:
 *
 *   set-up : r0 = b - A x0 ; r# = r0 ; u0 = u1 = u2 = 0 ; rho0 = 1, alpha = 0, omega = 1
 *            dot_zero = dot_r = (r0,r0) ; rho1 = (r#,r0)
 *   sweep  : rho0 = -omega rho0
 *     j=0  : beta = alpha (rho1 / rho0) ; rho0 = rho1 ; u0 = r0 - beta u0
 *            u1 = A u0 , (r#,u1)                         -> alpha = rho0 / (r#,u1)
 *            x += alpha u0 ; r0 -= alpha u1
 *            r1 = A r0 , (r#,r1)                         -> rho1
 *     j=1  : beta = alpha (rho1 / rho0) ; rho0 = rho1 ; u0 = r0 - beta u0 ; u1 = r1 - beta u1
 *            u2 = A u1 , (r#,u2)                         -> alpha = rho0 / (r#,u2)
 *            x += alpha u0 ; r0 -= alpha u1 ; r1 -= alpha u2
 *            r2 = A r1
 *     MR   : a11 = (r1,r1), a12 = (r1,r2), a22 = (r2,r2), b1 = (r0,r1), b2 = (r0,r2)
 *            det = a11 a22 - a12 a12 ; g1 = (b1 a22 - b2 a12) / det ; g2 = (a11 b2 - a12 b1) / det
 *            x += g1 r0 + g2 r1 ; r0 -= g1 r1 + g2 r2 ; u0 -= g1 u1 + g2 u2 ; omega = g2
 *            dot_r = (r0,r0) ; rho1 = (r#,r0) ; k += 2
 *
 * Every update is evaluated term by term from the left, one multiply and one add each, whatever the grid or the rank count; only the
 * association of the dot sums depends on them. Options and result fields keep their meaning:
 *   k            counts BiCG steps -- BICG_BICGSTAB's unit, one step = two products -- and advances by 2 per sweep.
 *   loop         a further sweep runs while dot_r > tol^2 dot_zero && k + 2 <= max_iter, evaluated on the device: k never exceeds
 *                max_iter (an odd max_iter = 7 ends at k <= 6; max_iter < 2 runs no sweep and returns k = 0 with x = x0).
 *   steps        bicg_run_iterate(n) enqueues ceil(n / 2) sweeps; check_every counts steps the same way. Sweeps enqueued behind a
 *                stopped solve change neither x, r nor any scalar.
 *   result       r comes back as the recursive residual; iterations, dot_r, dot_zero and the time fields as for BICG_BICGSTAB; the
 *                progress line is printed whenever k is a multiple of out_iter.
 *   breakdown    a non-finite alpha, beta, g1, g2 or dot_r ends the solve; breakdown_iteration is the k of the sweep it happened in
 *                (a 1 x 1 system ends this way in its first sweep). Nothing smarter is attempted.
 *   trace        entries k-2 and k-1 of a sweep hold the alpha and beta of its steps j = 0 and j = 1; omega[k-2] = g1 and
 *                omega[k-1] = g2; both dot_r entries hold the sweep's final (r0,r0), as does the history behind the progress lines.
 *   accepted by  bicg_solve, bicg_run, bicg_run_begin / _iterate / _iterate_timed / _end and bicg_solve_device, on one rank or several
 *                (collective as BICG_BICGSTAB). bicg_solve_multi / bicg_solve_multi_device return -2 for it.
 *   launches     always the multi-launch form with the producer-side finish: four products, six element-wise passes and five dot
 *                groups per sweep. Under BICG_GRAPH=1 it runs eagerly: the method has no captured iteration. It allocates nothing:
 *                its nine vectors (x, r#, r0, r1, r2, u0, u1, u2, the set-up's A x0) are the context's work vectors.
 * Out of scope: l > 2, multi-RHS sets, the persistent, hand-over and graph forms, shifted variants. (Preconditioned: methods 7 and 8.)
 *
 * BICG_BICGSTAB2_DIAG (7) and BICG_BICGSTAB2_BLOCK (8) -- the sweep above on A M^-1, right-preconditioned with the preconditioner the
 * context holds (bicg_precond_diagonal, kind 1, for method 7; bicg_precond_block_diagonal, kind 2, for method 8; DESIGN.md section
 * 4.24): for matrices that are convective AND badly scaled or block-coupled, on which methods 0, 4, 5 and 6 all fail. r0 stays the
 * residual of the caller's system A x = b, so the stopping test, k, the trace, the breakdown rule, the progress lines, check_every,
 * bicg_run_iterate(n) = ceil(n / 2) sweeps and "sweeps behind a stopped solve change neither x, r nor a scalar" are method 6's. Four
 * hat vectors ride along, u^0, u^1, r^0, r^1:
 *
 *   set-up : as method 6 (r0 = b - A x0 ; r# = r0 ; u0 = u1 = u2 = 0)
 *   sweep  : rho0 = -omega rho0
 *     j=0  : beta ; u0 = r0 - beta u0 ;                       u^0 = M^-1 u0          [application 1]
 *            u1 = A u^0 , (r#,u1) -> alpha
 *            r0 -= alpha u1 ;                                 r^0 = M^-1 r0          [application 2]
 *            r1 = A r^0 , (r#,r1) -> rho1
 *     j=1  : beta ; x += alpha u^0 (step j = 0's) ; u0 = r0 - beta u0 ;   u^0 = r^0 - beta u^0   [recurrence]
 *            u1 = r1 - beta u1 ;                              u^1 = M^-1 u1          [application 3]
 *            u2 = A u^1 , (r#,u2) -> alpha
 *            x += alpha u^0 ; r0 -= alpha u1 ;                r^0 -= alpha u^1       [recurrence]
 *            r1 -= alpha u2 ;                                 r^1 = M^-1 r1          [application 4]
 *            r2 = A r^1
 *     MR   : the five sums on r0, r1, r2 as above -> g1, g2
 *            x += g1 r^0 + g2 r^1 ; r0 -= g1 r1 + g2 r2 ; u0 -= g1 u1 + g2 u2 ; dot_r = (r0,r0) ; rho1 = (r#,r0) ; k += 2
 *
 * Four applications of M^-1 and two hat recurrences per sweep; the recurrences feed x alone -- every product's input is a fresh
 * application, so the recursive residual does not depend on them. Every expression is one multiply and one add per term from the
 * left, as above; a diagonal application is dinv_i v_i, a block application is bicg_precond_apply's. Consequences, bit for bit: with
 * d = 1 (or identity blocks) the sweep is method 6's; method 8 with bs = 1, or with blocks that hold d on their diagonals and zeros
 * elsewhere, is method 7 with that d (as long as no entry of a vector M^-1 is applied to is a zero, whose sign the two forms may
 * render differently).
 *   launches     method 7 forms the applications in the pass that produces the vector: ten launches per sweep, as method 6. Method 8
 *                follows each of those four passes with a launch of the block application, which writes the hat vector only:
 *                fourteen. Under BICG_GRAPH=1 both run eagerly. They allocate nothing: the hat vectors are the four work vectors
 *                method 6 leaves idle.
 *   accepted by  bicg_solve, bicg_run, bicg_run_begin / _iterate / _iterate_timed / _end and bicg_solve_device, on one rank or several
 *                (collective as method 6; blocks are local to a rank). On a context whose bicg_precond_kind is not the method's (1 /
 *                2) these calls return -2 and touch nothing. bicg_solve_multi / bicg_solve_multi_device return -2 for both.
 *   across ranks the refusal is a rank's own, as for methods 4 and 5: no rank asks another whether it holds the preconditioner. A rank
 *                whose preconditioner was cleared returns -2 at once and takes no part in the solve, while the ranks that hold one
 *                enter it and wait for that rank in their first collective. Installing on every rank, or on none, is the caller's
 *                contract.
 * Out of scope here: forming the block application in the producing pass (it needs out-of-place r0 / u1), l > 2, multi-RHS sets, the
 * persistent, hand-over and graph forms, CA / pipelined / shifted preconditioned forms, other preconditioner kinds. */

typedef struct {
    double tol;          /* relative residual tolerance, reference EPS (src/solver.c:3) */
    int    max_iter;     /* reference MAX_ITER (src/solver.c:4) */
    int    out_iter;     /* progress line every out_iter iterations, reference OUT_ITER (:9); 0 = never */
    int    check_every;  /* iterations enqueued between host convergence checks (device stops itself) */
    int    quiet;        /* 1: no stdout lines */
    int    krr, nrr;     /* residual replacement period / count (src/solver.c:433) */
    int    record_trace; /* 1: keep per-iteration alpha/omega/beta/(r,r) on the device */
    int    time_kernels; /* bit 0: give every SpMV kernel its own start/stop HIP events (roofline measurement);
                            bit 1: section timing -- the reference's MEASURE_SECTION_TIME (src/shifted_switching_solver.c:9,
                            src/shifted_solver.c:77-81, 230-247) on the device clock: an event wherever the kind of work changes
                            (product / element-wise / shifted systems / reduction hand-over), read with bicg_section_times.
                            Both keep the multi-launch forms (no persistent launch, no graph replay);
                            bit 2 (with bit 1; BICG_SECTION_TIME=2): the switching solvers also print the reference's
                            DISPLAY_SECTION_TIME table, one line per iteration, and its ten totals incl. "Switch time"
                            (src/shifted_switching_solver.c:884-892, 994-1005) */
    double rr_drift;     /* pipelined solvers, additive: > 0 enables ADAPTIVE residual
                            replacement -- at every host check the true residual b - A x is computed and, when
                            ||(b - A x) - r|| > rr_drift * ||r||, the next iteration is a replacement step
                            (the step of src/solver.c:498-508, 522-531). 0 = the reference's fixed krr/nrr policy only. */
} bicg_options;

typedef struct {
    int    iterations;     /* k, the reference's return value */
    double dot_r;          /* final (r,r), all ranks */
    double dot_zero;       /* (r0,r0) */
    double seconds;        /* wall time, init SpMV .. last iteration (the span of src/solver.c:70-131) */
    double iter_seconds;   /* wall time of the iteration loop only (after the set-up phase) */
    double spmv_ms_total;  /* sum of the kernel durations of all timed SpMVs (time_kernels) */
    int    spmv_launches;  /* number of SpMVs timed (an SpMV may consist of up to 4 kernels) */
    int    breakdown_iteration; /* first iteration with a non-finite alpha/beta/omega/(r,r); 0 = none.
                              The reference does not detect breakdown (it iterates on NaNs). */
    int    adaptive_replacements; /* replacement steps triggered by rr_drift */
} bicg_result;

void bicg_default_options(bicg_options *o);

/* Upload this rank's blocks and build the SpMV plan (row blocks, halo lists). Collective.
 * Returns NULL after printing to stderr on failure. The host arrays are not referenced afterwards. */
bicg_ctx *bicg_create(const CSR_Matrix *diag, const CSR_Matrix *offd, const INFO_Matrix *info);
void bicg_destroy(bicg_ctx *ctx);
/* Single rank, matrix ALREADY in device memory as CSR (device pointers, 32-bit indices, ptr_d[rows] = nnz): the sliced-ELL plan
 * is built by kernels, no host copy of the matrix is made -- what lets BASELINE.json configs[3] at its stated size (512^3
 * Laplacian: 134 M rows, 938 M non-zeros) be generated, planned and solved on ONE MI355X inside a bench run. The arrays are
 * not referenced after the call. plan_seconds (optional): wall time of the call. Returns NULL (after a line on stderr) for
 * blocks that need the host plan: ragged rows (jagged slices / x windows), long rows (rows over lanes), more than one rank.
 *   bicg_stencil7_device  CSR of the 7-point stencil on an m^3 grid in device memory (weights = centre, x-, x+, y-, y+, z-, z+;
 *                         entries in ascending column order: the matrix of the reference-style generator used by bench.py and
 *                         the tests, python/synth.py stencil7); arrays are released with bicg_device_free */
bicg_ctx *bicg_create_device_csr(const double *val_d, const unsigned int *col_d, const unsigned int *ptr_d, unsigned int rows,
                                 double *plan_seconds);
int bicg_stencil7_device(unsigned int m, const double *weights, double **val_d, unsigned int **col_d, unsigned int **ptr_d,
                         unsigned long long *nnz);
void bicg_device_free(void *p);

/* New values for the matrix of a context, same sparsity pattern: the values are written into the arrays that are already on the
 * device, at the positions the context's plan defines. Nothing is planned again; every device address of the context, its
 * iteration graphs, the probed pipelined choice, SpMM and multi-RHS buffers, traces, bicg_ctx_flags, bicg_plan_info,
 * bicg_device_matrix_bytes and the entry counts below stay what they were, and bicg_device_allocations() is the same after the
 * call as before it (the host variant's staging buffer is a temporary of the call; the device variant allocates nothing).
 *   diag_val[nnz_d], offd_val[nnz_o]  in the CSR order of the blocks handed to bicg_create -- the caller's numbering, also on a
 *                        BICG_FLAG_REORDERED context. offd_val may be NULL when the context has no offd entries; a rank without
 *                        rows passes empty arrays and the call does nothing. Contexts of bicg_create_device_csr are served too.
 *   the pattern          neither call takes one: that ptr / col are those of bicg_create is the CALLER'S CONTRACT, nothing checks it.
 * Local: no transport call, bicg_comm_counts does not move; across ranks every rank updates its own blocks before the next
 * collective call. The work is ordered on the context's compute stream behind everything already enqueued, and the call is
 * synchronised on return. The device variant reads its source arrays on that stream: they must be complete before the call (a
 * caller who fills them on a stream of its own synchronises that stream first).
 * Values held in shared lists are verified, never rewritten: constant and masked slices (bicg_constant_entries > 0) keep their
 * values in lists shared between slices, and whether a slice is constant is a property of its values. Before anything is written
 * every such slice is compared with the new values bit for bit; any difference refuses the call. A caller who WILL change such
 * values (e.g. the coefficients of a constant-coefficient stencil) creates the context under BICG_PLAN="constant=0", which also
 * disables masked slices. Unchanged ones -- identity rows of Dirichlet nodes in an otherwise varying matrix -- pass.
 * Returns 0: done; 1: refused (a list-held value would change), nothing written; -1: NULL context, or a NULL array where entries exist. */
int bicg_update_values(bicg_ctx *ctx, const double *diag_val, const double *offd_val);               /* host arrays   */
int bicg_update_values_device(bicg_ctx *ctx, const double *diag_val_d, const double *offd_val_d);    /* device arrays */
/* (Neither call touches a diagonal preconditioner installed with bicg_precond_diagonal below: a caller whose diagonal changed
 * installs it again, which costs one launch.) */

/* DIAGONAL PRECONDITIONER, M = diag(d), and the method that uses it. bicg_precond_diagonal installs or replaces it: the context keeps
 * 1.0 / d[i] on the device -- one correctly rounded division per row and nothing else.
 *   d            local_rows doubles in the CALLER'S numbering, also on a BICG_FLAG_REORDERED context (it crosses the permutation on
 *                the device, as the vectors of bicg_load_device do). Any diagonal: diag(A) (bicg_csr_diagonal, section 5), a lumped
 *                mass matrix, row norms. A rank without rows passes NULL.
 *   scope        local to the rank: no transport call, bicg_comm_counts does not move. Both variants are synchronised on return; the
 *                device variant first makes the compute stream wait for `stream` by an event, as the *_device calls below do, so a
 *                kernel that fills d_d on `stream` right before the call is complete before d_d is read. Not to be called between
 *                bicg_run_begin and bicg_run_end of ANY solve on the context, whatever its method: the quotients are formed in one
 *                of the context's work vectors (refused ones, infinities and NaNs among them, stay there until a solve overwrites it).
 *                Under BICG_GRAPH=1 the captured iteration of method 4 is dropped whenever the array of 1/d is made or freed.
 *   returns      0 installed; 1 refused -- some d[i] is zero or non-finite (checked on the device by the launch that divides): the
 *                previous preconditioner, or none, stays in place; -1 NULL context, or a NULL array where rows exist.
 *   lifetime     the first install allocates local_rows doubles (counted in bicg_device_allocations, released by bicg_destroy or
 *                bicg_precond_clear); later installs allocate nothing (the host variant's staging buffer is a temporary of the call).
 * bicg_precond_clear drops it (bicg_device_allocations() is back to what it was before the first install); bicg_precond_kind: 0 none,
 * 1 diagonal, 2 block diagonal (below).
 * BICG_BICGSTAB_DIAG is RIGHT preconditioning: the iteration runs on A M^-1, r stays the residual of the caller's system
 * A x = b and the stopping test (r,r) > tol^2 (r0,r0) is BICG_BICGSTAB's. The operations are those of reference src/solver.c:74-120
 * in their order, with p^ = (1/d) o p and q^ = (1/d) o q as the inputs of the two products and in the update of x; with d = 1 the
 * result is bit-identical to BICG_BICGSTAB's multi-launch form. Accepted by bicg_solve, bicg_run, bicg_run_begin / _iterate /
 * _iterate_timed / _end and bicg_solve_device; options, result fields, trace, progress and summary lines, breakdown detection and
 * check_every are BICG_BICGSTAB's. On a context WITHOUT a preconditioner these calls return -2 and touch nothing. Across ranks the
 * call is collective as for BICG_BICGSTAB; that every rank has installed its part is the caller's contract. It allocates nothing
 * beyond 1/d: the hat vectors live in work vectors the plain iteration leaves idle.
 * bicg_solve_multi / bicg_solve_multi_device accept it too (see there). Out of scope: the CA, pipelined and shifted iterations have
 * no preconditioned form. */
int bicg_precond_diagonal(bicg_ctx *ctx, const double *d_loc);                       /* host array   */
int bicg_precond_diagonal_device(bicg_ctx *ctx, const double *d_d, void *stream);    /* device array */
int bicg_precond_clear(bicg_ctx *ctx);
int bicg_precond_kind(bicg_ctx *ctx);

/* BLOCK-JACOBI PRECONDITIONER, M = the bs x bs diagonal blocks the caller passes, and the method that uses it (DESIGN.md section
 * 4.21). Several unknowns per node put a small dense block on the diagonal whose off-diagonal entries are as large as its diagonal
 * ones; the install inverts every block once, the iteration multiplies with the inverses.
 *   blocks       bs is 1..16. Block k covers this rank's local rows [k bs, min((k+1) bs, local_rows)) in the CALLER'S numbering, also
 *                on a BICG_FLAG_REORDERED context; nblocks = ceil(local_rows / bs); blocks[(k bs + a) bs + j] is entry (a, j) of block
 *                k, row-major, nblocks bs bs doubles (what bicg_csr_block_diagonal, section 5, writes). Of a partial last block only
 *                the leading m x m part is read (m = the rows it covers). A rank without rows passes NULL. Blocks are local to the
 *                rank; that they match the caller's unknowns is the caller's contract.
 *   returns      0 installed; 1 refused -- a block is singular or holds a non-finite entry (a pivot of the elimination is zero or
 *                non-finite, or the inverse overflows; checked on the device by the launch that inverts): whatever preconditioner was
 *                installed, of either kind, stays in place bit for bit; -1 NULL context, or a NULL array where rows exist; -2 bs
 *                outside 1..16, nothing is touched.
 *   inversion    Gauss-Jordan with partial pivoting per block (the entry of largest magnitude in the column among the rows not yet
 *                used, the first one on a tie), the pivot row scaled by one correctly rounded division per entry: bs = 1 keeps exactly
 *                1.0 / d, a diagonal block exactly 1.0 / d on its diagonal and zeros elsewhere.
 *   scope        as bicg_precond_diagonal: local to the rank (bicg_comm_counts does not move), synchronised on return, the device
 *                variant ordered behind `stream` by an event; not to be called between bicg_run_begin and bicg_run_end.
 *   lifetime     ONE preconditioner per context: a successful install of one kind releases the other kind's array. The context keeps
 *                bs planes of local_rows doubles (rounded up to whole 256-byte lines): one allocation, made by the first install, kept
 *                by later installs with the same bs, replaced by one with another bs; staging and the elimination's scratch are
 *                temporaries of the call. bicg_precond_clear drops whichever kind is installed; bicg_precond_kind returns 2 for this one.
 *                Under BICG_GRAPH=1 the captured iteration of method 5 is dropped whenever the planes are made, freed or replaced.
 * BICG_BICGSTAB_BLOCK is BICG_BICGSTAB_DIAG with p^ = M^-1 p and q^ = M^-1 q formed by a launch of their own (seven launches per
 * iteration instead of five; row i takes acc = m_0 v_0, then acc = fma(m_j, v_j, acc) over its block's rows in ascending order, whatever
 * the grid, the rank count or the layout). Accepted wherever method 4 is; options, result fields, trace, printed lines, breakdown
 * detection and check_every are BICG_BICGSTAB's. With bs = 1, or with blocks that hold d on their diagonals and zeros elsewhere, it is
 * bit-identical to method 4 with that d (as long as no entry of p or q is a zero, whose sign the two forms may render differently).
 * Method 5 on a context whose kind is not 2 returns -2 and touches nothing, as method 4 does on one whose kind is not 1.
 * bicg_solve_multi / bicg_solve_multi_device accept method 5 as well (see there): one launch per application for a whole set.
 * Out of scope: forming the hat vectors in the pass that produces p or q, the CA / pipelined / shifted iterations, blocks of
 * varying size. */
int bicg_precond_block_diagonal(bicg_ctx *ctx, const double *blocks, int bs);                          /* host array   */
int bicg_precond_block_diagonal_device(bicg_ctx *ctx, const double *blocks_d, int bs, void *stream);   /* device array */

/* Matrix residency of the drop-in entry points (section 1 and the shifted ones): the context of the last drop-in call
 * stays resident and is reused when the caller passes the same blocks again -- same arrays, sizes, partition,
 * communicator AND contents (a 64-bit hash over every value / column / row pointer: the matrix may have been edited in
 * place, e.g. by the reference's csr_shift_diagonal, src/matrix.c:518-531). The reference's drivers call a solver 10-28 x
 * on one matrix (src/main_repeat.c:109-132): only the first call pays for plan + upload. All ranks agree on hit / miss.
 * BICG_DROPIN_CACHE=0 in the environment restores create / destroy per call. BICG_DROPIN_CACHE=2 (opt-in): when every rank finds
 * the pattern unchanged and only values edited, the resident context takes them through bicg_update_values instead of being
 * re-created (still counted as a miss; a rank whose list-held values changed makes every rank re-create).
 *   bicg_dropin_context  the resident context for these blocks (created or reused; collective); owned by the library --
 *                        do NOT bicg_destroy it. Lets a host form b = A*1 with bicg_spmv and then call bicgstab() with
 *                        one upload (host/bicg_main.c)
 *   bicg_dropin_release  drop the resident context now (also happens in bicg_comm_finalize)
 *   bicg_dropin_stats    hits / misses so far
 *   bicg_dropin_refreshes  misses that were served by bicg_update_values (BICG_DROPIN_CACHE=2) */
bicg_ctx *bicg_dropin_context(const CSR_Matrix *diag, const CSR_Matrix *offd, const INFO_Matrix *info);
void bicg_dropin_release(void);
void bicg_dropin_stats(unsigned int *hits, unsigned int *misses);
unsigned int bicg_dropin_refreshes(void);

/* Whole solve with host vectors, semantics of section 1 (x_loc/r_loc in-out). */
int bicg_solve(bicg_ctx *ctx, int method, double *x_loc, double *r_loc, const bicg_options *opt,
               bicg_result *res);

/* Device-resident variant: load x0/b once, run, fetch. bicg_run leaves x and r on the device. */
int bicg_load(bicg_ctx *ctx, const double *x0_loc, const double *b_loc);
int bicg_run(bicg_ctx *ctx, int method, const bicg_options *opt, bicg_result *res);
int bicg_fetch(bicg_ctx *ctx, double *x_loc, double *r_loc);
/* The same solve in three steps (benchmarks time exactly K iterations this way):
 *   begin   = the reference's set-up phase (src/solver.c:74-83, 200-213, 333-348), synchronised
 *   iterate = up to nsteps further passes of its while loop (stops early on convergence or
 *             max_iter); returns k so far; synchronised on return
 *   end     = summary lines (src/solver.c:134-141) and result */
int bicg_run_begin(bicg_ctx *ctx, int method, const bicg_options *opt);
int bicg_run_iterate(bicg_ctx *ctx, int nsteps);
/* bicg_run_iterate with three clocks around it (ms): [0] the device's -- an event recorded on the compute stream in front of the
 * first launch and one behind the last (hipEventElapsedTime); [1] the host time spent enqueueing the launches (until the loop over
 * the iterations returned, before the scalars are fetched); [2] the host's wall time of the whole call. A region whose wall time
 * is long while [0] is not was held up on the host side (or between the queue and the device), not in the kernels. */
int bicg_run_iterate_timed(bicg_ctx *ctx, int nsteps, double ms[3]);
int bicg_run_end(bicg_ctx *ctx, bicg_result *res);
int bicg_sync(bicg_ctx *ctx);
/* shifted solve on a resident matrix; variant = BICG_SHIFTED_LOP / _PIPE / _XI / _FLAG / _SWITCH (semantics
 * of the drop-in functions above; opt NULL = reference defaults with EPS 1e-12); the trace holds the SEED
 * system's alpha, omega, beta, (r,r). _FLAG / _SWITCH (shifted_lopbicg / shifted_lopbicg_switching): the
 * return value follows the reference (the switching variants count from 1), bicg_result.iterations is the
 * number of iterations and bicg_result.adaptive_replacements the number of seed switches. */
enum { BICG_SHIFTED_LOP = 0, BICG_SHIFTED_PIPE = 1, BICG_SHIFTED_XI = 2, BICG_SHIFTED_FLAG = 3, BICG_SHIFTED_SWITCH = 4 };
int bicg_solve_shifted(bicg_ctx *ctx, int variant, double *x_loc_set, double *r_loc, const double *sigma, int sigma_len,
                       int seed, const bicg_options *opt, bicg_result *res);
/* The check of the reference's shifted driver (src/test_shifted.c:129-154) on the device: relres_out[j] =
 * || (A + sigma_j I) x_j - b || / || b || for every shift (x_loc_set shift-major as above). Collective. */
int bicg_shifted_residuals(bicg_ctx *ctx, const double *x_loc_set, const double *b_loc, const double *sigma, int sigma_len,
                           double *relres_out);
/* "Batched SpMV" (BASELINE.json configs[4]): Y_j = (A + sigma_j I) X_j for nvec vectors with every matrix entry read once
 * per 16 vectors (sliced-ELL SpMM) -- what the loop above does internally. x_loc_set / y_loc_set are shift-major like
 * x_loc_set of the shifted solvers; sigma may be NULL (Y_j = A X_j). Every column is bit-identical to bicg_spmv of that
 * vector. Padded and jagged slices, x-window slots and lane-permuted groups are all read (BICG_FLAG_SPMM). Where some rows are on
 * the CSR / rows-over-lanes kernels (a row several times longer than the average) there is no SpMM kernel: the columns are
 * multiplied one by one by bicg_spmv's kernels with the shift in their epilogue, A is read nvec times and ms_device receives 0.
 * ms_device (optional) otherwise receives the device time of the passes (halo exchanges, layout change and SpMM kernel).
 * Collective. */
int bicg_spmm(bicg_ctx *ctx, const double *x_loc_set, const double *sigma, int nvec, double *y_loc_set, double *ms_device);
/* per-iteration trace of the last run (record_trace): arrays of length >= iterations, may be NULL */
int bicg_trace(bicg_ctx *ctx, double *alpha, double *omega, double *beta, double *dot_r);
/* Plain BiCGStab on nrhs independent systems A x_j = b_j that share the resident matrix: one SpMM per product for up to 16
 * columns, every column with its own alpha / omega / beta and its own convergence test. Methods: BICG_BICGSTAB (0), and its
 * right-preconditioned forms BICG_BICGSTAB_DIAG (4) on a context whose bicg_precond_kind is 1 and BICG_BICGSTAB_BLOCK (5) on one
 * whose kind is 2 -- the preconditioned methods are described behind the plain one below.
 * x_loc_set / r_loc_set are column-major, [j * local_rows + i], like x_loc_set of the shifted solvers: in = x0_j and b_j, out =
 * the solution and the recursive residual of column j. Column j runs exactly the loop of reference src/solver.c:74-120 on
 * (x0_j, b_j), with the loop condition dot_r > tol*tol*dot_zero && k < max_iter evaluated per column ON THE DEVICE at every
 * iteration: a column whose condition has become false (a NaN in its scalars included) is frozen -- its x_j and r_j are not
 * written again whatever the other columns go on doing --, and no column influences another. The dot products of a column are
 * summed in an order that depends on local_rows only, so column j of any call is bit-identical to a one-column call on
 * (x0_j, b_j). nrhs > 16 is processed as consecutive sets of 16 columns (the last one may be partial).
 * opt->check_every iterations are enqueued between host reads of the columns' flags; opt->record_trace keeps alpha, omega, beta
 * and (r,r) per column and iteration for bicg_multi_trace (max_iter x 16 x 4 doubles per set). res (nrhs entries, may be NULL):
 * iterations, dot_r, dot_zero and breakdown_iteration of column j; the time fields of every entry are those of the whole call.
 * Returns the largest k_j; -2 for methods 1-3 and 6-8, for method 4 or 5 on a context whose bicg_precond_kind is not that method's (1 / 2),
 * or for nrhs < 1 -- a refused call touches nothing: neither x, r, the trace nor any allocation.
 * METHODS 4 AND 5: column j runs exactly the right-preconditioned iteration bicg_solve runs for that method on (x0_j, b_j): the two
 * products take P^ = M^-1 P and Q^ = M^-1 Q, x += alpha p^ + omega q^, r stays the residual of the caller's system, and the loop
 * condition, freezing, check_every, record_trace, bicg_multi_trace, the res entries, sets of 16 with a partial last one, the per-column
 * product fallback and the collective rules below are the plain call's. With d = 1, or identity blocks of any bs, every column is
 * bit-identical to the plain call. The preconditioner is read as installed at the time of the call: one re-installed or replaced
 * between two calls takes effect in the second. Launches: method 4 makes the plain call's, the hat vectors being written by the
 * passes that produce p and q; method 5 adds ONE launch per application for the whole set (k_bjac_apply_set: a row's bs plane
 * entries are loaded once for the 16 columns; every column gets the bytes bicg_precond_apply gives on it; frozen columns are neither
 * read nor written), i.e. two launches per iteration and set, and one behind the set-up phase. Memory: the first preconditioned
 * call on a context makes ONE more allocation, the two hat sets (2 x 16 vectors, 32 x 8 bytes per row), zeroed once; later calls of
 * any method allocate nothing; bicg_destroy releases it.
 * Across ranks a rank whose context lacks the method's preconditioner returns -2 and the other ranks return -1, nothing is touched
 * anywhere (the rule for ld < local_rows of bicg_solve_multi_device); bs and the blocks are a rank's own and need not agree.
 * The products are SpMMs that read P and R in place where bicg_spmm is available (BICG_FLAG_SPMM) and one bicg_spmv-style product
 * per active column otherwise, or under BICG_PLAN="spmm=0" (read at the call). Memory: the first call allocates six sets of 16
 * vectors beside the SpMM's own buffers -- 96 x 8 bytes per row, about 1.2 GB at 1.6 M rows --, released by bicg_destroy.
 * COLLECTIVE when the communicator has more than one rank: every rank calls with the same method, nrhs, max_iter, check_every
 * and tol (ranks without rows pass nrhs and empty arrays). The call begins with a check of exactly that, one all-reduce in which
 * every rank takes part whatever its own arguments are: -1 means the ranks did NOT pass the same arguments (or do not agree on
 * BICG_PLAN="spmm=0") -- every rank returns -1 and nothing is touched; when they agree and the arguments are refusable every rank
 * returns -2. Per product a set costs ONE halo exchange (the 16 halos packed peer-major; BICG_PLAN="halo-set=0", read at the
 * call, or a peer-to-peer context: one per column), per dot group ONE all-reduce of nranks x 32 doubles that gathers every
 * rank's local sums -- each rank's row is added to zeros only, which is exact --, after which every rank adds the rows in the same
 * fixed order (the association of a recursive-doubling all-reduce, ascending rank order up to three ranks).
 * What is bit-identical to what, across ranks: (a) k, dot_r, dot_zero, breakdown_iteration and the trace of a column are the same bytes on every rank, so all ranks take the same decisions; (b) column j of any call is bit-identical to a one-column
 * collective call on (x0_j, b_j) at the same partition, whatever check_every is; (c) the result does not depend on the
 * transport's summation order, on halo-set, or on spmm=0. It is NOT bit-identical to the one-rank call: the partition decides
 * how a column's dot sums are associated (as it does for the reference under MPI). One rank: unchanged.
 * On a peer-to-peer context (bicg_comm_enable_p2p) the products use the peer-to-peer halo path, one exchange per column, while
 * the all-reduces of the dot groups go through the transport underneath: correct, not optimised. */
int bicg_solve_multi(bicg_ctx *ctx, int method, double *x_loc_set, double *r_loc_set, int nrhs,
                     const bicg_options *opt, bicg_result *res /* nrhs entries, may be NULL */);
/* trace of column `column` of the last bicg_solve_multi call run with record_trace: arrays of length >= that column's
 * iterations, may be NULL. Returns 0; non-zero when nothing was recorded or the column is out of range. */
int bicg_multi_trace(bicg_ctx *ctx, int column, double *alpha, double *omega, double *beta, double *dot_r);

/* DEVICE-RESIDENT VECTORS: the calls above for a caller whose vectors are in device memory. Every pointer is a device pointer to
 * fp64 on the context's device, 8-byte aligned, in the CALLER'S numbering also on a BICG_FLAG_REORDERED context; `stream` is the
 * caller's hipStream_t (NULL: the null stream). Apart from where the vectors live the semantics are those of the host variants,
 * and what they return is bit-identical to the host variant's on the same context: k, x, r, the result fields and the traces.
 *   bicg_load_device         fills the context's x and r; bicg_run and bicg_run_begin / _iterate / _end then work unchanged.
 *                            x0_d == NULL keeps the x the context already holds (warm start: a time stepper starts from the
 *                            previous solution without moving it) -- defined when the last call that wrote the context's x was
 *                            a bicg_load* or a bicg_run* / bicg_solve* on it. b_d is always required: a solve overwrites r.
 *   bicg_fetch_device        either pointer may be NULL, as in bicg_fetch.
 *   bicg_solve_device        load + solve + fetch; x_d / r_d in-out.
 *   bicg_spmv_device         the collective product y = A x; y_d must not alias x_d.
 *   bicg_solve_multi_device  bicg_solve_multi with column j at set + j * ld, ld >= local_rows, columns in-out. Collectivity,
 *                            return values, freezing, the res entries, the traces and the memory behaviour are bicg_solve_multi's;
 *                            a refused call touches neither set.
 * Stream ordering, both ways, without a host synchronisation added by the crossing: before the library touches the caller's arrays
 * it records an event on `stream` and makes its compute stream wait for it; after the last kernel that reads or writes them it
 * records an event on the compute stream and makes `stream` wait for it. So what the caller enqueued on `stream` before the call
 * (the kernel that fills b_d) is complete before the arrays are read, and what it enqueues on `stream` after the call is ordered
 * behind it: b_d may be overwritten on `stream` right after bicg_load_device, x_d read on `stream` right after bicg_fetch_device,
 * and a caching allocator that recycles memory in stream order stays safe. Work on OTHER streams is the caller's to order. The
 * solving calls synchronise with the host where the host variants do, at their convergence checks; bicg_spmv_device ends with the
 * host variant's check of the peers on a peer-to-peer context and otherwise returns without a host wait; load and fetch never wait.
 * The calls must NOT be made while `stream` is being captured into a graph.
 * The crossing is one launch (csrc/bicg_vecio.hip) and allocates nothing -- no staging buffer, also on a reordered context:
 * bicg_device_allocations() is the same after load / fetch / solve / spmv as before, and bicg_solve_multi_device allocates what
 * bicg_solve_multi does on a context's first multi call and nothing later. A rank without rows passes NULL (or empty) arrays,
 * takes part in every collective and copies nothing.
 * Return: 0 done (the solving calls: their k); -1 NULL context, or a NULL required array where rows exist; -2 as bicg_solve_multi,
 * and for ld < local_rows. Across ranks a rank whose own arrays bicg_solve_multi_device has to refuse still takes part in the
 * call's argument check, and the other ranks then return -1 as for any disagreement. */
int bicg_load_device(bicg_ctx *ctx, const double *x0_d, const double *b_d, void *stream);
int bicg_fetch_device(bicg_ctx *ctx, double *x_d, double *r_d, void *stream);
int bicg_solve_device(bicg_ctx *ctx, int method, double *x_d, double *r_d, const bicg_options *opt, bicg_result *res, void *stream);
int bicg_spmv_device(bicg_ctx *ctx, const double *x_d, double *y_d, void *stream);
int bicg_solve_multi_device(bicg_ctx *ctx, int method, double *x_set_d, double *r_set_d, size_t ld, int nrhs,
                            const bicg_options *opt, bicg_result *res /* nrhs entries, may be NULL */, void *stream);

/* ---------------------------------------------------------------------------------------------
 * 4. Kernel-level entry points (parity tests, benchmarks).
 *   bicg_spmv        <- MPI_csr_spmv_ovlap, reference src/matrix.c:428-441 (collective)
 *   bicg_dot         <- my_ddot + MPI_Iallreduce, reference src/vector.c:9-15, src/solver.c:89-91
 * ------------------------------------------------------------------------------------------- */
int bicg_spmv(bicg_ctx *ctx, const double *x_loc, double *y_loc);
/* z = M^-1 v for the installed preconditioner (kind 1 or 2); host arrays, caller's numbering, local to the rank; z may alias v.
 * Returns 0 done, -2 none installed (or a NULL context). Uses two of the context's work vectors: not between bicg_run_begin and
 * bicg_run_end. The operator by itself, for tests and for a flexible outer iteration of the caller's. */
int bicg_precond_apply(bicg_ctx *ctx, const double *v_loc, double *z_loc);
/* reps back-to-back applications of the installed preconditioner on device-resident vectors; returns average ms per application
 * (HIP events on the library's compute stream), as bicg_spmv_bench does for the product. 0 done, -2 none installed. */
int bicg_precond_apply_bench(bicg_ctx *ctx, int reps, double *ms_per_apply);
/* the same for the set application of bicg_solve_multi's method 5: ncols (1..16) columns per launch, average ms per launch. chunk:
 * columns a workgroup walks, 4, 8 or 16, anything else the library's choice -- for measuring that choice. 0 done; -2 no block
 * preconditioner installed, or ncols out of range. Allocates what a first preconditioned bicg_solve_multi call allocates. */
int bicg_precond_apply_set_bench(bicg_ctx *ctx, int ncols, int chunk, int reps, double *ms_per_apply);
double bicg_dot(bicg_ctx *ctx, const double *x_loc, const double *y_loc);
/* reps back-to-back SpMVs on device-resident vectors; returns average ms per SpMV (HIP events on
 * the library's compute stream) */
int bicg_spmv_bench(bicg_ctx *ctx, int reps, double *ms_per_spmv);
/* STREAM-style bandwidth of THIS GPU, the denominator north_star prices the SpMV against ("measure
 * its own STREAM-triad/copy on the box"): kind 0 copy a = b, 1 triad a = b + s c (both 16-byte accesses), 2 read-only with
 * 8-byte loads, 3 read-only with 16-byte loads. bytes_per_array should exceed the 256 MiB Infinity Cache several times
 * (bench.py: 1 GiB). gbps = bytes read + written per second; ms = one pass. Returns 0. Needs a GPU. */
int bicg_stream_bench(int kind, unsigned long long bytes_per_array, int reps, double *gbps, double *ms);
/* 1 after a peer-to-peer wait of this context timed out (only reachable with BICG_P2P_SOFT_FAIL=1; the
 * default is to print the error and exit like any other HIP/RCCL failure). The solve in progress stops. */
int bicg_comm_failed(bicg_ctx *ctx);
/* Transport collectives issued for this context since bicg_create: out = {halo exchanges (the transport's exchange of device
 * buffers: one per bicg_spmv-style product, one per SET of vectors in bicg_spmm / bicg_shifted_residuals / bicg_solve_multi),
 * all-reduces (one per dot group; one per dot group of a whole set in bicg_solve_multi)}. Host counters, incremented where the
 * calls are made: exchanges and sums that travel on the peer-to-peer data path are not transport calls and are not counted, and
 * a rank with neither halo nor send list issues no exchange. Returns 0. */
int bicg_comm_counts(bicg_ctx *ctx, unsigned long long out[2]);
/* How long the exchanges of the last solve made the persistent kernels wait (multi-rank, peer-to-peer data path): one sample per
 * exchange, taken on the device clock inside the launch. out = {all-reduce of a dot group through the mailboxes: p50, p99; a
 * boundary workgroup's wait from publishing its own values to a complete window, the neighbour's halo values included: p50, p99
 * (microseconds); number of samples of either}. Returns 0 when something was recorded. What a first multi-GPU run needs to
 * explain itself: the links' latency as the kernels saw it (reference overlap: src/solver.c:363-367, src/matrix.c:432-440). */
int bicg_comm_wait_stats(bicg_ctx *ctx, double out[6]);
/* Section times of the last solve run with bicg_options.time_kernels & 2 (BICG_SECTION_TIME=1 in the drop-in path), in
 * milliseconds on the compute stream: ms[0] element-wise kernels of the seed system (with their fused dots), ms[1] products
 * A x (halo exchange and joins of overlapped all-reduces included), ms[2] the passes over the shifted systems (the shifted
 * solvers print "Seed time" / "Shift time" like the reference: shift = ms[2], seed = total - shift,
 * src/shifted_solver.c:230-247), ms[3] reduction hand-overs that are launches of their own (host / RCCL all-reduce + apply,
 * peer-to-peer collect); with one rank the scalars are applied inside the producing kernels and ms[3] is 0.
 * *iterations = iterations covered, *marks = events used (negative: the pool of 65536 ran out and timing stopped there).
 * Returns 0, or 2 when the last solve was not timed. */
int bicg_section_times(bicg_ctx *c, double ms[4], int *iterations, int *marks);

/* plan facts: local rows, diag nnz, offd nnz, halo length, workgroups per SpMV, halo-touching
 * workgroups, rows on the sliced-ELL path, sliced-ELL padding entries */
int bicg_plan_info(bicg_ctx *ctx, unsigned int out[8]);
/* which code paths this context takes (tests assert on them): peer-to-peer data path in use; halo exchange
 * folded into the sliced-ELL SpMV launch; two-stream overlap mode; 16-bit column offsets; every 256-row
 * group on the sliced-ELL path; jagged slices (ragged rows, no padding stored); bicg_spmm available (the same
 * on every rank); x windows in LDS with 16-bit slots instead of column indices; rows spread over lanes */
enum { BICG_FLAG_P2P = 1, BICG_FLAG_LL_FUSED = 2, BICG_FLAG_OVERLAP = 4, BICG_FLAG_COL16 = 8, BICG_FLAG_ALL_SELL = 16, BICG_FLAG_JAGGED = 32,
       BICG_FLAG_SPMM = 64, BICG_FLAG_WINDOW = 128,
       BICG_FLAG_ROWSPLIT = 256   /* long rows: a row is spread over 8..64 lanes (k_spmv_rows); row sums then agree with the
                                     reference's to 1e-13 x sum |a_ij x_j| instead of bit for bit */,
       BICG_FLAG_PERSIST = 512    /* pipe_bicgstab runs as ONE persistent launch per chunk of iterations (latency-bound ranks:
                                     matrix slices and x window in LDS, vectors in registers; bicg_persist.hip) */,
       BICG_FLAG_FUSE_PIPE = 1024 /* multi-launch pipelined iterations run their element-wise phases in the SpMV epilogues (two
                                     launches per iteration) rather than as separate kernels */,
       BICG_FLAG_PIPE_PROBED = 2048 /* ... and that was MEASURED on this matrix by the first pipelined solve (BICG_PLAN="pipe-probe")
                                     instead of decided by the size / layout rule of bicg_create */,
       BICG_FLAG_UNIFORM = 4096   /* some 64-row slices are UNIFORM -- all rows present, equally long, entry k at the same distance
                                     from its row in every row (the interior of a banded or stencil matrix): the SpMV takes their
                                     columns from one shared list of distances and reads no column index for them (8 instead of
                                     10 / 12 bytes per non-zero); bicg_uniform_entries counts those entries */,
       BICG_FLAG_CONSTANT = 8192  /* ... and some of them are CONSTANT: entry k also holds the same value in all 64 rows (the interior
                                     of a constant-coefficient stencil such as the 7-point Laplacian of BASELINE.json configs[3]):
                                     the values come from a shared list too and the slice streams nothing from the matrix arrays;
                                     bicg_constant_entries counts those entries. Same products, same order: bit-identical */,
       BICG_FLAG_REORDERED = 16384 /* BICG_PLAN="reorder=1|2": bicg_create renumbered the diag block (P A P^T, reverse Cuthill-McKee,
                                     one rank only) before planning it; every vector the caller hands in or gets back crosses the
                                     permutation on the device, so the caller keeps its own numbering. The entries of a row keep
                                     their stored order: products stay bit-identical to mult() on the caller's matrix */,
       BICG_FLAG_HANDOVER = 32768  /* plain BiCGStab on this context closes its dot groups by hand-over: the producing kernel leaves
                                     shard totals, the kernel that consumes the scalars adds them and applies the recurrence
                                     (one rank, padded 16-bit layout; BICG_PLAN="handover=0" selects the producer-side finish).
                                     Same sums, same order: bit-identical */,
       BICG_FLAG_TAIL_FINISH = 65536 /* ticket-mode dot groups whose workgroups come from ONE launch close by the tail finish (the
                                     launch's last workgroups add the partial sums); clear under BICG_TAIL_FINISH=0, hipGraph replay
                                     and the peer-to-peer transport: every group then closes by arrival tickets, as a group that
                                     spans several launches always may. Same sums, same order: bit-identical */ };
unsigned int bicg_ctx_flags(bicg_ctx *ctx);
/* The reordering of a context with BICG_FLAG_REORDERED: the stats of bicg_reorder_plan (section 5) with out[7] = microseconds
 * bicg_create spent on ordering + permuting. Returns 0; 1 and zeros when the context is not reordered. */
int bicg_reorder_info(bicg_ctx *ctx, unsigned long long out[8]);
/* bytes of MATRIX storage this context keeps on the GPU (CSR and/or sliced-ELL arrays, row pointers, offd block) */
unsigned long long bicg_device_matrix_bytes(bicg_ctx *ctx);
/* sliced-ELL entries (padding included) whose column indices the SpMV does not read (BICG_FLAG_UNIFORM), and the bytes one
 * SpMV streams from the matrix arrays (values + the column indices it does read + row pointers) */
unsigned long long bicg_uniform_entries(bicg_ctx *ctx);
unsigned long long bicg_constant_entries(bicg_ctx *ctx);
/* rows of MASKED slices: slices next to a grid face, whose rows are sub-sequences of one list of <= 16 (distance, value) pairs;
 * the product reads one 16-bit word per row for them (which pairs the row has) instead of values and columns. Counted in
 * bicg_uniform_entries / bicg_constant_entries too (with their padded entries). BICG_PLAN="masked=0" switches them off */
unsigned long long bicg_masked_rows(bicg_ctx *ctx);
/* The plane-marching product (csrc/bicg_stencil.hip): when the plan finds the 7-point stencil of a grid in the lists of a block
 * whose slices are all list-driven -- the interior's distances are (-sz, -sy, -1, 0, +1, +sy, +sz) with sy a multiple of 64 rows,
 * sz a multiple of sy, the rows a multiple of sz, and every other list a sub-sequence of that one -- y = A x runs with every
 * wavefront marching through the planes of its own grid lines (BASELINE.json configs[3]); same sums in the same order as
 * mult() (reference src/matrix.c:506-515). out = {in use (0/1), sy, sz / sy, rows / sz, lines per wavefront, planes per tile,
 * workgroups per product, x segments with masked slices}. BICG_PLAN="stencil=0" switches it off (slice-by-slice product);
 * BICG_PLAN="lines=2|4,planes=n" sets the tile; BICG_PLAN="ca-fuse=0" keeps CA-BiCGStab's q / y phase a kernel of its own */
int bicg_stencil_info(bicg_ctx *ctx, unsigned int out[8]);
/* Rows per lane of the plane-marching product: 1 (k_spmv_stencil), 2 or 4 (k_spmv_stencil_w: a wavefront's line is 128 / 256 rows,
 * one pair of edge lines per line instead of one per 64 rows; taken when every list of the block has the same value per distance --
 * constant-coefficient stencils -- and the vectors exceed the Infinity Cache, or BICG_PLAN="wide=2|4" asks for it; "wide=0" keeps
 * one row per lane). 0 when the product is not in use. Same sums as mult(), reference src/matrix.c:506-515. */
unsigned int bicg_stencil_rows_per_lane(bicg_ctx *ctx);
/* bicg_create_device_csr groups its list-driven slices by 64-bit hashes of their lists and then compares every slice with the
 * list it was given: the number of slices that did NOT match (hash collisions) and were put back on their stored columns and
 * values. 0 for contexts built by bicg_create (the host plan keys on the full lists). */
unsigned int bicg_plan_collisions(bicg_ctx *ctx);
/* Device allocations this process has made through the library's host code and not yet freed: the contexts' matrix, plan,
 * vectors and lazily grown buffers (traces, shift sets, SpMM / multi-RHS sets, staging) and the temporaries of a call in progress.
 * Not counted: the transports' own memory (the landing ring among it) and what bicg_stencil7_device hands to the caller. The
 * count after bicg_destroy equals the count before the matching bicg_create, whatever was called in between. */
long long bicg_device_allocations(void);
/* Which product kernels this process has launched since the last call with reset != 0 (bit mask): 1 k_spmv_sell on padded slices,
 * 2 k_spmv_sell on jagged slices (columns gathered through the caches), 4 k_spmv_sell's loop over jagged slices with the x window
 * in LDS, 8 k_spmv_jagw (the three-trip form of that product, csrc/bicg_jagw.hip), 16 k_spmv_stencil, 32 k_spmv (CSR row blocks),
 * 64 k_spmv_rows (a row over several lanes), 128 a product with a pipelined phase in its epilogue,
 * 512 k_spmv_jagd (the three-trip product of jagged slices without a window: x gathered through the caches), 1024 k_spmv_jagw with a
 * list-driven window (the group's distinct columns one by one). Tests and bench.py assert on the kernel a matrix gets. */
unsigned int bicg_product_kernels(int reset);
/* 1 when the last bicg_solve_shifted / shifted_pipe_lopbicgstab call on this context ran its iterations as persistent launches
 * (k_shpipe_persist: latency-bound ranks, <= 32 shifts; BICG_PERSIST="shifted=0" keeps the multi-launch form) */
int bicg_last_shifted_persistent(bicg_ctx *ctx);
/* Which kernel the last bicg_spmm / bicg_shifted_residuals pass on this context ran: 2 the pipelined one (k_spmm_pipe,
 * csrc/bicg_spmm.hip: the x window of the next step copied global -> LDS by the DMA path while the current step multiplies,
 * persistent workgroups; padded 16-bit layouts whose distances fall into clusters), 1 the windowed one (k_spmm_win: the x values a
 * 256-row group touches staged in LDS through registers; BICG_PLAN="spmm-window=1" selects it everywhere, and layouts with x-window
 * runs take it), 0 the row-major kernel k_spmm_sell (BICG_PLAN="spmm-window=0", and layouts without clusters or window runs).
 * In all three the vectors' columns are bit-identical to bicg_spmv of each vector. */
int bicg_last_spmm_windowed(bicg_ctx *ctx);
/* Rows per tile of that pass when it ran k_spmm_pipe: 512, or 256 (the window does not fit 512-row tiles, or
 * BICG_TEST="spmm-tile=256"); 0 after any other kernel (k_spmm_jpipe, k_spmm_win, k_spmm_sell). Read-only. */
int bicg_last_spmm_tile(bicg_ctx *ctx);
unsigned long long bicg_spmv_matrix_bytes(bicg_ctx *ctx);

/* ---------------------------------------------------------------------------------------------
 * 5. Host-only helpers (no GPU needed; unit-tested on CPU).
 *   bicg_partition   <- reference src/matrix.c:295-308
 *   bicg_halo_plan   -- unique global columns referenced by an offd block, grouped by owner rank
 * ------------------------------------------------------------------------------------------- */
void bicg_partition(unsigned int n, int nranks, int *counts, int *displs);
/* The diagonal of a diag block (local columns): d_out[i] = the stored (i,i) entry, 0.0 where none is stored; a row that stores
 * (i,i) more than once yields their sum in stored order. Returns the number of rows without one. What bicg_precond_diagonal takes
 * for a Jacobi preconditioner (after the caller has dealt with the rows that have none). */
int bicg_csr_diagonal(const CSR_Matrix *diag, double *d_out);
/* The bs x bs diagonal blocks of a diag block (local columns) in the layout bicg_precond_block_diagonal takes (ceil(rows / bs) bs bs
 * doubles): entry (i, j) with i / bs == j / bs lands at its place, an entry stored more than once yields the sum in stored order,
 * everything else is 0.0. Returns the number of rows without a stored (i,i) entry (information only: a block without one may well be
 * regular); -2 for bs outside 1..16, nothing written. With bs = 1 the output is bicg_csr_diagonal's. */
int bicg_csr_block_diagonal(const CSR_Matrix *diag, int bs, double *blocks_out);
/* Returns the halo length h and fills (caller-allocated, sizes noted):
 *   halo_cols[offd->nz upper bound]  ascending unique global columns
 *   recv_counts[nranks]              how many of them each rank owns
 *   renumbered[offd->nz]             offd->col mapped to local_rows + halo position */
int bicg_halo_plan(const CSR_Matrix *offd, const INFO_Matrix *info, int nranks, unsigned int local_rows,
                   unsigned int *halo_cols, int *recv_counts, unsigned int *renumbered);
/* Collective (through the caller's alltoallv): the SEND side of the halo exchange, in two steps.
 * Given this rank's halo_cols/recv_counts from bicg_halo_plan:
 *   bicg_halo_send_counts fills send_counts[nranks] (how many of OUR rows each rank needs) and
 *                         returns their sum;
 *   bicg_halo_send_lists  fills send_idx[sum] with the local row indices, grouped by destination
 *                         rank; returns the sum, or -1 if a peer asked for a row we do not own. */
int bicg_halo_send_counts(int nranks, const int *recv_counts, bicg_alltoallv_fn alltoallv, void *user,
                          int *send_counts);
int bicg_halo_send_lists(int rank, int nranks, const INFO_Matrix *info, unsigned int local_rows,
                         const unsigned int *halo_cols, const int *recv_counts, const int *send_counts,
                         bicg_alltoallv_fn alltoallv, void *user, unsigned int *send_idx);
/* greedy row blocks of at most chunk non-zeros (whole rows); returns the number of blocks and fills
 * rowblk[nblk+1] (caller provides rows+1 entries) */
unsigned int bicg_row_blocks(const unsigned int *ptr, unsigned int rows, unsigned int chunk,
                             unsigned int max_rows, unsigned int *rowblk);
/* x windows of the sliced-ELL plan for ragged rows: for every group of group_rows rows
 * (group_mask[g] != 0, or all when NULL) the columns its rows touch, merged into runs of consecutive columns
 * (gaps of <= gap unused columns are bridged). runs[2i] = first column, runs[2i+1] = (first slot << 16) | length;
 * win_ptr[g] .. win_ptr[g+1] index a group's runs; *slots_used = slots of the largest window. Returns the
 * number of runs, -1 when a group needs more than max_slots slots. runs / win_ptr / slots_used may be NULL
 * (count only). bicg_window_slot: the slot of column c in the window runs[2*first .. 2*end). */
long bicg_window_plan(const unsigned int *ptr, const unsigned int *col, unsigned int rows, unsigned int group_rows,
                      const char *group_mask, unsigned int max_slots, unsigned int gap, unsigned int *win_ptr,
                      unsigned int *runs, unsigned int *slots_used);
unsigned int bicg_window_slot(const unsigned int *runs, unsigned int first, unsigned int end, unsigned int c);
/* Host threads of the set-up (bicg_create's plan and bicg_window_plan cut their loops over slices / groups / rows into one range
 * per thread; the results do not depend on the number). 0 < n: use n threads from now on; n < 0: back to the default; returns the
 * number in use. Default: BICG_PLAN_THREADS, else the hardware threads this process may run on (its affinity mask) divided by the
 * ranks that share the host (LOCAL_WORLD_SIZE / OMPI_COMM_WORLD_LOCAL_SIZE / MPI_LOCALNRANKS / SLURM_NTASKS_PER_NODE, else the
 * communicator's size), at most 32. */
int bicg_set_plan_threads(int n);

/* Plan of the persistent iteration (host only, what bicg_create builds for latency-bound ranks): the
 * workgroups' slices as padded entries {value, 16-bit slot of the column in the workgroup's window}, diag entries first, then
 * the offd entries (offd_renumbered: columns = local rows + halo position as bicg_halo_plan renumbers them; NULL for one rank),
 * and the window runs {first column, (first slot << 16) | length} per workgroup. gmax = workgroups available (CUs - 1).
 * summary = {slices per workgroup, workgroups, window slots, most runs of a workgroup, most entries of a workgroup, entries,
 * runs, 0}; arrays may be NULL (sizes: a first call). Returns 0 when the block qualifies (<= 15 slices per workgroup, windows
 * within 16 384 slots). */
int bicg_persist_plan(const CSR_Matrix *diag, const CSR_Matrix *offd_renumbered, unsigned int gmax, unsigned int summary[8],
                      unsigned int *pbase, unsigned short *pslot, double *pval, unsigned short *rlen, unsigned short *rdiag,
                      unsigned int *win_ptr, unsigned int *win_runs);
/* ... and where every entry of its pval came from (same arguments and qualification): psrc[e] = index into (diag values followed
 * by offd values) of pval[e], 0xFFFFFFFF for padding; as many entries as pval (summary[5]). bicg_update_values refills the
 * persistent plan through this map. Returns 0 when the block qualifies. */
int bicg_persist_plan_sources(const CSR_Matrix *diag, const CSR_Matrix *offd_renumbered, unsigned int gmax, unsigned int *psrc);
/* The sliced-ELL plan of a diag block (host only, what bicg_create plans before it uploads anything), read
 * with the switches of the environment, as numbers a test can pin. diag: this rank's diag block; offd_renumbered: its offd block
 * (only the row pointers are read: which rows touch the halo), NULL for one rank; rows_global / nnz_diag_global: rows and diag
 * non-zeros of ALL ranks (what bicg_create learns from its first collective).
 * summary = {0 jagged layout, 1 16-bit column offsets, 2 fused-window clusters, 3 x windows (0 none, 1 runs, 2 list-driven),
 *   4 group selection retried, 5 rows over lanes, 6 sliced-ELL entries, 7 their non-zeros, 8 their rows, 9 uniform entries,
 *   10 constant entries, 11 masked rows, 12 CSR row blocks, 13 interior groups, 14 halo-touching groups, 15 CSR-order 16-bit
 *   offsets, 16 window slots, 17 most runs of a window, 18 windows within 16 bits of their group, 19 most entries of a jagged
 *   slice behind its rows' 16th, 20 halo-touching row blocks, 21 lane info present}.
 * digest = 64-bit FNV-1a over the bytes of {0 slice_len, 1 slice_base, 2 slice_base16, 3 sval, 4 scol, 5 scol16, 6 perm,
 *   7 group_is_sell, 8 gl_int, 9 gl_bnd, 10 bint, 11 bbnd, 12 win_ptr, 13 win_runs, 14 list, 15 lptr, 16 total, 17 ubase, 18 vbase,
 *   19 mbase, 20 uoff, 21 uval, 22 rmask, 23 lane_info, 24 dcol16, 25 the FusedWindow} (an array the plan does not have: the
 *   digest of no bytes). Returns 0 on success. */
int bicg_sell_plan_digest(const CSR_Matrix *diag, const CSR_Matrix *offd_renumbered, int nranks, unsigned int rows_global,
                          unsigned long long nnz_diag_global, unsigned long long summary[22], unsigned long long digest[26]);
/* The launch plan of one distributed product y = A x (host only, what every product of every solver asks
 * before it enqueues anything): which launches the product consists of and how their workgroups share the dot group's partial
 * slots, as numbers a test can pin. Needs no context and no device; reads no environment.
 * shape = {0 interior sliced-ELL groups, 1 halo-touching groups, 2 interior CSR row blocks, 3 halo-touching row blocks, 4 row
 *   blocks in all, 5 every group on the sliced-ELL path, 6 transport (0 one rank, 1 peer-to-peer, 2 hosted), 7 the exchange can
 *   ride inside the sliced-ELL launch, 8 this rank sends halo values, 9 the hosted exchange runs on its own stream, 10 the
 *   plane-marching product is available, 11 its workgroups, 12 groups per workgroup, 13 ... of a product with dots, 14 workgroup
 *   cap of ranks sharing a GPU (0: none)}.
 * call = {0 fused dots, 1 epilogue (0 none, 1 / 2 pipelined phases, 3 CA-BiCGStab's q / y), 2 shifted product, 3 the dot group
 *   carries a tail tag, 4 it is a per-wavefront group}.
 * plan = {0 error (0 none, 1 epilogue 3 without the plane-marching product on one rank, 2 epilogue on a product of several
 *   launches, 3 the plane-marching launch would decline), 1 groups per workgroup, 2 plane-marching, 3 exchange inside the launch,
 *   4 one launch over all groups, 5 partial slots the group expects, 6 shard totals of a hand-over group, 7 the group's partial
 *   count is set from 5, 8 the tail finish stays, 9 steps}; with an error, entries from 5 on say nothing.
 * steps = 4 rows of {0 kernel family (0 sliced-ELL, 1 sliced-ELL with epilogue, 2 plane-marching, 3 CSR row blocks), 1 list
 *   (0 all groups, 1 interior groups, 2 halo-touching groups, 3 the fused list, 4 interior row blocks, 5 halo-touching row
 *   blocks), 2 entries of the list, 3 reads the offd block, 4 exchange inside, 5 first partial slot, 6 runs after the halo has
 *   landed}, in launch order; rows from plan[9] on are zero. Returns 0, 1 for a null array or an unknown transport. */
int bicg_spmv_launch_plan(const unsigned int shape[15], const int call[5], unsigned int plan[10], unsigned int steps[28]);
/* Who closes a dot group (host only, what every solver asks when it opens a group): what the producer's
 * reduction descriptor says and the ordered operations that turn the group's sums into applied scalars, as numbers a test can
 * pin. Needs no context and no device; reads no environment.
 * shape = {0 transport (0 one rank, 1 peer-to-peer, 2 hosted), 1 the hosted collectives run in stream order, 2 two streams
 *   (BICG_OVERLAP), 3 peer-to-peer: the producer's last workgroup may collect and apply, 4 tail finish switched on, 5 iterations
 *   are replayed from a captured graph, 6 hand-over switched on and possible on this matrix}.
 * call = {0 regime (0 tickets / tail finish, 1 consumer-side finish, 2 hand-over), 1 sums, 2 their offset in Scal::red, 3 phase,
 *   4 one rank: the producer applies the recurrence, 5 event (0 a group that closes at once, 1 one deferred across the next
 *   product, 2 the host or a product needs the open group's scalars before a consumer came, 3 the consuming kernel's launch, 4 a
 *   producer that neither opens nor closes), 6 the group open when the call is made (0 none, 1 open, 2 deferred and not yet
 *   staged, 3 staged by a product), 7 the call comes from a product}.
 * plan = {0 error (0 none, 1 a group produced while one is open, 2 a product with dots asked to stage a deferred group, 3 a
 *   hand-over consumer without a group), 1-3 the producer's Reduce: wave, hand, apply_now, 4 its p2p.n_collect, 5 it carries a new
 *   tail tag, 6 it publishes to the peers' mailboxes, 7 the group rides across the next product, 8 steps}.
 * steps = 7 rows of {0 operation (0 nothing: the producer's last workgroup did it, 1 stand-alone finish, 2 all-reduce, 3 k_apply,
 *   4 k_apply_p2p, 5 event recorded on the stream, 6 the stream waits for the event recorded last, 7 staged by the next product's
 *   first launch, 8 finished by the consuming kernel), 1 when (0 at close, 1 behind the next product's halo start, 2 after that
 *   product, 3 in the consumer), 2 stream (0 compute, 1 communication), 3 FIN_* roles, 4 sums, 5 offset, 6 phase}, in order; rows
 *   from plan[8] on are zero. Returns 0, 1 for a null array or an entry outside its range. */
int bicg_dot_group_plan(const int shape[7], const int call[8], int plan[9], int steps[49]);

/* Bandwidth-reducing renumbering of a diag block (host only, what bicg_create does under
 * BICG_PLAN="reorder=1|2"). Reverse Cuthill-McKee on the symmetrised pattern (entry (i, j) makes i and j neighbours whichever of
 * the two is stored; the diagonal is ignored): one breadth-first sweep per connected component from its lowest-numbered vertex of
 * minimum degree, components in ascending order of that vertex, within a level by (parent's position, degree, original index),
 * each component's order reversed; rows without neighbours last, in their original order. A pure function of the pattern.
 * perm[new] = old for the diag block (rows entries, caller-allocated). method: 1 = RCM. stats = {0 rows, 1 connected components,
 * 2 bandwidth max|i-j| as given, 3 after, 4 most distinct columns of a 256-row group as given, 5 after, 6 rows without
 * neighbours, 7 0}. Returns 0. */
int bicg_reorder_plan(const CSR_Matrix *diag, int method, unsigned int *perm, unsigned long long stats[8]);
/* P A P^T with the stored entry order of every row kept; out arrays caller-allocated (rows + 1, nz, nz). Returns 0, -1 when
 * perm is not a permutation of 0..rows-1. */
int bicg_permute_block(const CSR_Matrix *diag, const unsigned int *perm, unsigned int *ptr_out, unsigned int *col_out, double *val_out);

/* Matrix-Market block loader (host only): what MPI_csr_load_matrix_block produces for `rank` of
 * `nranks` (reference src/matrix.c:402-419) -- diag block with local columns, offd block with global
 * columns, file order inside a row, equal-rows partition -- reading the file once. Arrays are
 * malloc'ed; release with bicg_mtx_free. Returns 0 on success. (The C host additionally has an MPI
 * variant in which every rank tokenises 1/P of the file, mpi-bicgstab_amd/host/bicg_mtx.h.) */
int bicg_mtx_load_block(const char *path, int rank, int nranks, CSR_Matrix *diag, CSR_Matrix *offd, INFO_Matrix *info);
/* The "next" pieces of the ingest path, host only:
 *   bicg_partition_nnz        contiguous row blocks with equal non-zero counts (idea of the reference's
 *                             abandoned DYNAMIC_ROWS branch, archive/matrix.c:407-446); the solver accepts
 *                             any contiguous partition through INFO_Matrix.recvcounts/displs
 *   bicg_mtx_load_block_part  the loader above with part = BICG_PART_ROWS | BICG_PART_NNZ
 *   bicg_mtx_cache_save/load  checksummed binary copy of one rank's parsed blocks; load returns 0 on a
 *                             valid hit for exactly this (rank, nranks, part) and unchanged source file */
/*   bicg_mtx_parse_double    the loader's conversion of one value: returns 0 when its own exact fast path (Eisel-Lemire,
 *                             <= 19 significant digits) produced it, 1 when it was handed to strtod; either way *value is
 *                             what fscanf("%lg") gives (src/matrix.c:333) and *consumed the characters used */
enum { BICG_PART_ROWS = 0, BICG_PART_NNZ = 1 };
void bicg_partition_nnz(const unsigned int *row_nnz, unsigned int n, int nranks, int *counts, int *displs);
int bicg_mtx_parse_double(const char *text, double *value, int *consumed);
int bicg_mtx_load_block_part(const char *path, int rank, int nranks, int part, CSR_Matrix *diag, CSR_Matrix *offd,
                             INFO_Matrix *info);
int bicg_mtx_cache_save(const char *cache_path, const char *src_path, int rank, int nranks, int part,
                        const CSR_Matrix *diag, const CSR_Matrix *offd, const INFO_Matrix *info);
int bicg_mtx_cache_load(const char *cache_path, const char *src_path, int rank, int nranks, int part,
                        CSR_Matrix *diag, CSR_Matrix *offd, INFO_Matrix *info);
void bicg_mtx_free(CSR_Matrix *diag, CSR_Matrix *offd, INFO_Matrix *info);
/* Device-side COO -> CSR (needs a GPU): the triplets this rank owns -- FILE order, global row and column
 * indices, rows in [lo, hi) -- become the diag block (local columns) and the offd block (global columns,
 * cols = ncols) that MPI_csr_load_matrix_block yields (reference src/matrix.c:336-392), file order kept inside
 * every row (a stable sort on the row key, like the reference's merge sort, src/matrix.c:135-183).
 * Arrays are malloc'ed; release with free() / bicg_mtx_free. bicg_mtx_set_block_builder(fn) makes the
 * Matrix-Market loaders above use fn for that step (NULL = host counting sort); the C host does so with
 * BICG_INGEST=device. */
typedef int (*bicg_block_builder_fn)(const unsigned int *row, const unsigned int *col, const double *val, unsigned long nnz,
                                     unsigned int lo, unsigned int hi, unsigned int ncols, CSR_Matrix *diag, CSR_Matrix *offd);
int bicg_coo_to_blocks_device(const unsigned int *row, const unsigned int *col, const double *val, unsigned long nnz,
                              unsigned int lo, unsigned int hi, unsigned int ncols, CSR_Matrix *diag, CSR_Matrix *offd);
void bicg_mtx_set_block_builder(bicg_block_builder_fn fn);

const char *bicg_version(void);
/* 1: the library was built with `make EXPERIMENTS=1` and reads the measurement knobs of the development rounds (csrc/bicg_knobs.h;
 * the negative results they select -- window-fused plain iteration, direct SpMM -- are compiled in); 0: the default build */
int bicg_has_experiments(void);
/* What the library reads from one of its token-list variables (BICG_PLAN, BICG_PERSIST, BICG_TEST: comma-separated `name` or
 * `name=value` tokens): copies the value of token `name` in $set to out ("1" for a bare token) and returns
 * its length, -1 when the variable or the token is absent. No device needed. */
int bicg_switch_value(const char *set, const char *name, char *out, int cap);
/* Tokens of $set that are none of the names the library knows for it (a typing error selects nothing): copies the first one to out
 * and returns their number. bicg_create prints one line per list on rank 0 when there are any. */
int bicg_switch_unknown(const char *set, char *out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* BICGSTAB_HIP_H */
