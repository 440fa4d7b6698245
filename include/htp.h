/* htp.h -- C ABI of the MI355X-native headland-turn planner (libhtp.so).
 *
 * Drop-in boundary for the OBCA hot path of AgRoboticsResearch/
 * headland_trajectory_planning.  The reference has no FFI of its own (it is
 * pure Python over CasADi/IPOPT); these entry points replace:
 *
 *   htp_obca_solve_batch   OBCAOptimizer(...).solve()   R/obca_py/optimizer.py:77-138 (NLP
 *                          construction) + :475-571 (nlpsol("ipopt") + solution slicing),
 *                          batched over independent problems.
 *   htp_obca_sizes         the decision-variable / constraint counts printed at
 *                          R/obca_py/optimizer.py:490-498.
 *
 * Ownership: every array is caller-owned.  htp_obca_solve_batch takes HOST
 * pointers (the library stages them to HBM); htp_obca_solve_batch_device takes
 * DEVICE pointers already resident in HBM.  The library owns its workspace.
 * Errors: 0 = OK, < 0 = API error (message via htp_last_error); per-problem
 * solver status in htp_obca_result.status (HTP_STATUS_*).  No exceptions cross
 * the ABI.  One htp_ctx per host thread.
 */
#ifndef HTP_H_
#define HTP_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HTP_NPARAM 24
/* per-problem parameter slots (double params[batch][HTP_NPARAM]) */
enum {
  HTP_P_DT = 0, HTP_P_Q00, HTP_P_Q01, HTP_P_Q10, HTP_P_Q11, HTP_P_R00, HTP_P_R01, HTP_P_R10, HTP_P_R11,
  HTP_P_W00, HTP_P_W11, HTP_P_WHEELBASE, HTP_P_MAXSTEER, HTP_P_MAXV, HTP_P_MAXACC, HTP_P_MAXSR,
  HTP_P_DMIN, HTP_P_XLO, HTP_P_XHI, HTP_P_YLO, HTP_P_YHI, HTP_P_HAS_INIT_CONTROL, HTP_P_HAS_INIT_DUAL
};

enum {
  HTP_STATUS_SUCCESS = 0,            /* IPOPT "Solve_Succeeded" */
  HTP_STATUS_ACCEPTABLE = 1,         /* "Solved_To_Acceptable_Level" */
  HTP_STATUS_MAX_ITER = 2,           /* "Maximum_Iterations_Exceeded" */
  HTP_STATUS_RESTORATION_FAILED = 3, /* "Restoration_Failed" */
  HTP_STATUS_STEP_FAILED = 4,        /* "Error_In_Step_Computation" */
  HTP_STATUS_BAD_INPUT = 5,          /* "Invalid_Problem_Definition" */
  HTP_STATUS_CPUTIME = 6,            /* "Maximum_CpuTime_Exceeded" (option max_cpu_time, device clock) */
  HTP_STATUS_INFEASIBLE = 7,         /* "Infeasible_Problem_Detected" (restoration converged, infeasible) */
  HTP_STATUS_TINY_STEP = 8           /* "Search_Direction_Becomes_Too_Small" */
};

typedef struct htp_ctx htp_ctx;

/* One batch of OBCA problems sharing N (horizon), M obstacles, K bodies and
 * the per-polytope edge counts.  Layouts are row-major, problem-major. */
typedef struct {
  int32_t batch, N, M, K, time_opt;   /* time_opt = (W[1][1] != 0), optimizer.py:109 */
  const int32_t* obs_edges;           /* [M] edges of each obstacle polytope (<= 8)  */
  const int32_t* body_edges;          /* [K] edges of each body polytope (<= 8)      */
  const double* traj;                 /* [batch][N][5] init_traj (x, y, v, theta, steer) */
  const double* obs_A;                /* [batch][sum obs_edges][2]  A of A x <= b    */
  const double* obs_b;                /* [batch][sum obs_edges]                      */
  const double* body_G;               /* [batch][sum body_edges][2] G of G x <= g    */
  const double* body_g;               /* [batch][sum body_edges]                     */
  const double* params;               /* [batch][HTP_NPARAM]                         */
  const double* init_control;         /* nullable [batch][N-1][2]                    */
  const double* init_mu;              /* nullable [batch][N][mu_count]               */
  const double* init_lambda;          /* nullable [batch][N][lambda_count]           */
} htp_obca_batch;

typedef struct {
  double* x;            /* [batch][n_var] optimal decision vector, optimizer.py layout */
  double* objective;    /* [batch] f(x*) (unscaled) */
  int32_t* status;      /* [batch] HTP_STATUS_* */
  int32_t* iterations;  /* [batch] IPM iterations */
  int32_t* n_factor;    /* [batch] KKT factorizations (inertia-correction retries included) */
  double* nlp_error;    /* [batch] final scaled NLP error */
  int32_t* n_resto;     /* nullable [batch] feasibility restoration phases entered */
} htp_obca_result;

/* Sizes of one problem (n_var, n_eq, n_ineq as printed by optimizer.py:490-498)
 * and the solver workspace in doubles. */
int htp_obca_sizes(int32_t N, int32_t M, int32_t K, int32_t time_opt, const int32_t* obs_edges,
                   const int32_t* body_edges, int64_t* n_var, int64_t* n_eq, int64_t* n_ineq,
                   int64_t* ws_doubles);

htp_ctx* htp_create(int32_t device);
void htp_destroy(htp_ctx* ctx);
const char* htp_last_error(htp_ctx* ctx);
/* IPOPT option override by name (e.g. "tol", "max_iter", "max_cpu_time" = seconds per problem on the
 * device wall clock, <= 0 off); 0 = OK */
int htp_set_option(htp_ctx* ctx, const char* name, double value);

/* Host buffers in, host buffers out (synchronous). */
int htp_obca_solve_batch(htp_ctx* ctx, const htp_obca_batch* in, htp_obca_result* out);
/* Device-resident buffers in/out; enqueued on `stream` (hipStream_t, may be
 * NULL = default stream).  Not synchronised. */
int htp_obca_solve_batch_device(htp_ctx* ctx, const htp_obca_batch* in, htp_obca_result* out, void* stream);
/* Average duration (ms) of the last solve kernel measured with hipEvents on
 * the launch stream (used by bench.py for the roofline). */
double htp_last_kernel_ms(htp_ctx* ctx);
 /* Diagnostic: per-problem shader-cycle counters of the last solve, [batch][8]:
 * local sweeps, assembly, stage chain, KKT solves, total, errors+grad_lag, line search, update. */
int htp_last_cycles(htp_ctx* ctx, int64_t* out, int32_t batch);

/* Work queue of problem indices feeding ONE persistent solve launch (no
 * reference counterpart: the reference solves one problem per Python call;
 * this is the batch runtime behind bench.py's multi-GPU work stealing,
 * SURVEY.md 8(e)).  The queue lives in pinned, GPU-coherent host memory: the
 * host appends problem indices and closes it; each wavefront of the running
 * launch claims the next ticket with a device atomic, waits until that ticket
 * is published (or the queue is closed: then it retires), and solves problem
 * items[ticket].  Per-ticket results go to out->objective/status/... [ticket];
 * out->x is indexed by problem.  A wave that waits longer than
 * `max_wait_s` for a ticket retires (status of that ticket stays unwritten). */
typedef struct htp_queue htp_queue;
htp_queue* htp_queue_create(htp_ctx* ctx, int64_t capacity);
void htp_queue_destroy(htp_queue* q);
/* Append problem indices (0 <= pid < batch of the launch); -1 when full / closed. */
int htp_queue_publish(htp_queue* q, const int32_t* pids, int64_t n);
int htp_queue_close(htp_queue* q);
int64_t htp_queue_published(const htp_queue* q);
/* Tickets claimed so far by the launch's waves (a monotone lower bound). */
int64_t htp_queue_claimed(const htp_queue* q);
/* Enqueue the persistent launch on `stream` over the device-resident inputs of
 * `in` (in->batch = number of resident problems); `waves` = wavefronts in the
 * launch (<= 0: as many as fit on the device at once). */
int htp_obca_solve_queue_device(htp_ctx* ctx, const htp_obca_batch* in, htp_queue* q, htp_obca_result* out,
                                void* stream, int32_t waves, double max_wait_s);
/* Wavefronts of the OBCA solve kernel resident on the device at once. */
int32_t htp_obca_resident_waves(htp_ctx* ctx, const htp_obca_batch* in);

/* ---------------------------------------------------------------------------
 * Point formulation (R/obca_py/optimizer_points.py OBCAOptimizer: initialize_manual
 * :52-108, generate_object :193-227, generate_variable :229-255, generate_constrain
 * :257-327, solve :157-191): lambda-only duals, one distance row per vehicle hull
 * vertex, hard start/end states, objective sum du^2 + 20 (v dT)^2.  Same solver,
 * batched; x in optimizer_points.py's variable order (X, U, LAMBDA obstacle-major).
 * Parameters: HTP_P_DT, _WHEELBASE, _MAXSTEER, _MAXV (MAX_VELOCITY), _MAXACC,
 * _MAXSR (MAX_STEER_RATE), _DMIN (MIN_DISTANCE_TO_OBS), _XLO.._YHI (min/max x/y);
 * the Q/R/W slots are ignored (the reference never reads r, q). */
typedef struct {
  int32_t batch, N, M, n_vertices;
  const int32_t* obs_edges;   /* [M] halfspaces of each obstacle = len(obstacle) (<= 8) */
  const double* traj;         /* [batch][N][5] init_guess_path */
  const double* obs_A;        /* [batch][sum obs_edges][2] compute_polytope_halfspaces A */
  const double* obs_b;        /* [batch][sum obs_edges]                                 */
  const double* vertices;     /* [batch][n_vertices][2] get_vehicle_vertices (:35-50)   */
  const double* params;       /* [batch][HTP_NPARAM]                                    */
  const double* init_control; /* nullable [batch][N-1][2]                               */
} htp_obca_points_batch;

int htp_obca_points_sizes(int32_t N, int32_t M, int32_t n_vertices, const int32_t* obs_edges, int64_t* n_var,
                          int64_t* n_eq, int64_t* n_ineq, int64_t* ws_doubles);
/* host buffers in/out (synchronous) */
int htp_obca_points_solve_batch(htp_ctx* ctx, const htp_obca_points_batch* in, htp_obca_result* out);
/* device-resident buffers, enqueued on `stream`; timing via htp_last_kernel_ms */
int htp_obca_points_solve_batch_device(htp_ctx* ctx, const htp_obca_points_batch* in, htp_obca_result* out,
                                       void* stream);

/* ---------------------------------------------------------------------------
 * Audit of solved OBCA trajectories (no reference counterpart for the optimised
 * trajectory: R/obca_py/optimizer.py:501-571 returns the last iterate of a solve
 * whatever its status, and its collision rows :386-425 hold MIN_DISTANCE_TO_OBS
 * only at the N stage nodes, through the duals; the reference's planners check
 * warm starts on densely sampled poses with check_path_feasibility).  For every
 * problem of a batch the audit places the body polygons at the poses of the
 * trajectory and measures, by geometry alone, the signed distance to every
 * obstacle polygon (Euclidean distance when disjoint, minus the penetration
 * depth when they intersect); it never reads mu, lambda or the slack.
 *   Poses: the nodes i = 0..N-1 and, with substeps = S > 1, S-1 poses inside every
 *   interval, from the NLP's own integrator started at X_i with step h q / S,
 *   h = dT tau_i (midpoint rule with time_opt, :367-370; Euler otherwise, :372-373).
 *   `in` is the struct the solve took (init_control / init_mu / init_lambda are
 *   ignored); x has the solve's n_var stride and optimizer.py's layout; only X, U
 *   and tau are read.  One wavefront per problem, the whole batch in one launch. */
#define HTP_AUDIT_MAX_SUBSTEPS 16
#define HTP_AUDIT_MAX_N 480          /* horizon the kernel's LDS staging holds */
enum {                               /* double metrics[batch][HTP_AUDIT_NMETRIC] */
  HTP_AUDIT_CLEARANCE = 0,           /* min signed distance over all poses and (obstacle, body) pairs */
  HTP_AUDIT_CLEARANCE_NODE,          /* the same over the N nodes only */
  HTP_AUDIT_DYN_DEFECT,              /* max |X_{i+1} - F(X_i, U_i, tau_i)|, the rows of :364-377 */
  HTP_AUDIT_BOUND_EXCESS,            /* largest violation of the generate_variables bounds :292-354 (X, U, tau); 0 if none */
  HTP_AUDIT_INIT_MISS,               /* max |X_0 - init_traj[0]| (the solver's init state, :358) */
  HTP_AUDIT_TERM_MISS,               /* max |X_{N-1} - init_traj[N-1]| (the solver's end state, :381) */
  HTP_AUDIT_PATH_LENGTH,             /* sum |v_i| h_i */
  HTP_AUDIT_TOTAL_TIME,              /* sum h_i */
  HTP_AUDIT_NMETRIC
};
enum {                               /* int32 flags[batch], judged against the caller's tolerances */
  HTP_AUDIT_COLLISION = 1,           /* clearance < 0 */
  HTP_AUDIT_MARGIN = 2,              /* clearance < params[HTP_P_DMIN] - margin_tol */
  HTP_AUDIT_DYNAMICS = 4,            /* defect > dyn_tol */
  HTP_AUDIT_BOUNDS = 8,              /* excess > bound_tol */
  HTP_AUDIT_TERMINAL = 16,           /* term_tol > 0 and the terminal miss exceeds it */
  HTP_AUDIT_NONFINITE = 32,          /* a non-finite double among those read: metrics NaN, worst -1, no other flag */
  HTP_AUDIT_BAD_POLYTOPE = 64        /* an empty or unbounded obstacle or body: clearance metrics NaN, worst -1 */
};
typedef struct {
  int32_t substeps;                  /* 1 (nodes only) .. HTP_AUDIT_MAX_SUBSTEPS */
  double margin_tol, dyn_tol, bound_tol, term_tol;   /* >= 0; term_tol = 0 switches HTP_AUDIT_TERMINAL off */
} htp_obca_audit_opts;
typedef struct {
  double* metrics;          /* [batch][HTP_AUDIT_NMETRIC] */
  int32_t* worst;           /* [batch][4] stage, substep, obstacle, body of HTP_AUDIT_CLEARANCE; ties go to the
                               lowest (stage, substep, obstacle, body) */
  int32_t* flags;           /* [batch] HTP_AUDIT_* bits */
  double* stage_clearance;  /* nullable [batch][N]: min over substeps and pairs for node i and the interval it starts */
} htp_obca_audit_result;
/* API errors (-1 with a message, nothing launched): a null argument, N < 2 or > HTP_AUDIT_MAX_N, substeps
 * outside 1..HTP_AUDIT_MAX_SUBSTEPS, an edge count outside 3..8, a negative tolerance.  batch == 0 returns 0. */
/* host pointers, synchronous */
int htp_obca_audit_batch(htp_ctx* ctx, const htp_obca_batch* in, const double* x, const htp_obca_audit_opts* opts,
                         htp_obca_audit_result* out);
/* device pointers, enqueued on `stream`, not synchronised: behind htp_obca_solve_batch_device on the same
 * stream it audits that solve's out->x without a host round trip */
int htp_obca_audit_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const double* x,
                                const htp_obca_audit_opts* opts, htp_obca_audit_result* out, void* stream);
/* duration (ms) of the last audit kernel (hipEvents on its stream) */
double htp_obca_audit_last_ms(htp_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Uniform-time sampling of solved OBCA trajectories (no reference counterpart:
 * R/obca_py/optimizer.py:501-571 returns the N nodes of the NLP's own grid, whose
 * spacing h_i = dT tau_i differs per interval with time optimisation, :235).  For
 * every problem of a batch the sampler returns the trajectory at the fixed period
 * dt, by the NLP's own integrator (midpoint rule with time_opt, :367-370; Euler
 * otherwise, :372-373) started at the node that opens the interval of each sample.
 *   Node times t_0 = 0, t_{i+1} = t_i + h_i and node arc lengths A_0 = 0,
 *   A_{i+1} = A_i + |v_i| h_i are serial left-to-right sums (the order of
 *   HTP_AUDIT_TOTAL_TIME and HTP_AUDIT_PATH_LENGTH); T = t_{N-1}.
 *   Regular rows: k = 0, 1, .. while k dt < T, at s = k dt (a product, never
 *   accumulated); interval i = the largest i in 0..N-2 with t_i <= s; state =
 *   step(X_i, U_i, s - t_i); arc = A_i + |v_i| (s - t_i).  Then exactly one final
 *   row: the stored node X_{N-1} with U_{N-2}, t = T, arc = A_{N-1}, stage N-1.
 *   The end of interval i and node i+1 differ by the solve's dynamics defect
 *   (HTP_AUDIT_DYN_DEFECT); the sampler does not hide that step.
 *   `in` is the struct the solve took; only X, U and tau of x and the dT and
 *   wheelbase parameters are read.  One wavefront per problem, one launch. */
#define HTP_TIMELINE_NCOL 10         /* t, x, y, v, theta, steer, accel, steer_rate, curvature, arc */
#define HTP_TIMELINE_MAX_N HTP_AUDIT_MAX_N
enum {                               /* int32 flags[batch] */
  HTP_TIMELINE_TRUNCATED = 1,        /* rows needed > cap: the first cap rows are written (possibly without the
                                        final row); count still holds the rows needed */
  HTP_TIMELINE_NONFINITE = 2,        /* a non-finite double among those read: count 0, no row written, no other flag */
  HTP_TIMELINE_BAD_TIME = 4          /* some h_i is not > 0, or T / dt >= 2^30: count 0, no row written */
};
typedef struct {
  double dt;                         /* output period, finite and > 0 */
  int32_t cap;                       /* rows of storage per problem, >= 2 */
} htp_obca_timeline_opts;
typedef struct {
  double* rows;             /* [batch][cap][HTP_TIMELINE_NCOL]; rows at or beyond min(count, cap) are never written */
  int32_t* stage;           /* nullable [batch][cap]: the interval i of a regular row, N-1 for the final row */
  int32_t* count;           /* [batch] rows needed = regular rows + 1 */
  int32_t* flags;           /* [batch] HTP_TIMELINE_* bits */
  double* duration;         /* nullable [batch] T; NaN where the h_i are non-finite or not all > 0 */
} htp_obca_timeline_result;
/* API errors (-1 with a "[timeline]" message, nothing launched): a null required argument, N < 2 or
 * > HTP_TIMELINE_MAX_N, dt not finite or <= 0, cap < 2, an edge count outside 3..8.  batch == 0 returns 0. */
/* host pointers, synchronous; only [X | U | tau] of every x row is uploaded */
int htp_obca_timeline_batch(htp_ctx* ctx, const htp_obca_batch* in, const double* x,
                            const htp_obca_timeline_opts* opts, htp_obca_timeline_result* out);
/* device pointers, enqueued on `stream`, not synchronised: behind htp_obca_solve_batch_device (and the audit)
 * on the same stream it samples that solve's out->x without a host round trip */
int htp_obca_timeline_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const double* x,
                                   const htp_obca_timeline_opts* opts, htp_obca_timeline_result* out, void* stream);
/* duration (ms) of the last timeline kernel (hipEvents on its stream) */
double htp_obca_timeline_last_ms(htp_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Repair of solves that lose the margin between nodes (no reference counterpart: the OBCA rows of
 * R/obca_py/optimizer.py:386-425 hold MIN_DISTANCE_TO_OBS at the N nodes and nowhere else, so a successful
 * solve may still carry HTP_AUDIT_COLLISION or HTP_AUDIT_MARGIN).  A flagged problem is solved again with its
 * margin raised by its own deficit, warm-started from its own X, U, mu and lambda, audited against the
 * ORIGINAL margin, and its result is kept where the dense clearance grew.  Two steps, pack and merge, and the
 * loop that runs them around htp_obca_solve_batch_device and htp_obca_audit_batch_device.
 *   Per-problem state (htp_obca_repair_state): all-zero arrays are a fresh state.  A problem is RETIRED once it
 *   carries RESOLVE_FAILED or GAVE_UP.  dmin_used is read only where rounds_used > 0.
 *   Pack.  Problem p is a candidate when out->status[p] is 0 or 1, audit->flags[p] has COLLISION or MARGIN and
 *   neither NONFINITE nor BAD_POLYTOPE, and p is not retired.  Its next margin is
 *     dmin_cur + (dmin_orig - clearance) + pad          (doubles, left to right)
 *   with dmin_orig = in->params[p][HTP_P_DMIN], dmin_cur = dmin_used[p] (dmin_orig before the first round) and
 *   clearance = audit->metrics[p][HTP_AUDIT_CLEARANCE].  A candidate whose next margin is not
 *   <= dmin_orig + max_raise is not packed: it gets CANDIDATE | GAVE_UP.  The others get CANDIDATE and are numbered
 *   in ascending problem order: count = their number, index[s] = the problem of slot s, and slot s < cap receives
 *   a complete htp_obca_batch row: traj (rows 1..N-2 = X_i of out->x, rows 0 and N-1 the rows of in->traj, bit for
 *   bit: they are the NLP's start and end state), init_control = U, init_mu / init_lambda = the mu / lambda blocks
 *   of out->x, the four polygon arrays, params_audit = in->params[p], params = the same with HTP_P_DMIN = the next
 *   margin and both HTP_P_HAS_INIT_* slots 1.  With count > cap the first cap slots are written; slots at or beyond
 *   min(count, cap) never are.  The solver has no input for tau: a re-solve starts at tau = 1, as the reference's
 *   solver does.
 *   Merge.  `re` / `re_audit`: the solve of the packed batch and its audit made with params_audit (slot-major).
 *   Slot s < min(count, cap) is ADOPTED if and only if re->status[s] is 0 or 1, re_audit->flags[s] has neither
 *   NONFINITE nor BAD_POLYTOPE and no bit outside COLLISION | MARGIN that audit->flags[p] lacks, and its
 *   HTP_AUDIT_CLEARANCE is strictly larger than the adopted one.  An adopted slot replaces out->x[p] (the whole row),
 *   every result field and every audit row of p = index[s]; adopted[s] = 1.  In every case dmin_used[p] = the
 *   slot's margin, rounds_used[p] += 1, extra_iterations[p] += re->iterations[s], and state[p] gains IMPROVED
 *   (adopted), REPAIRED (adopted and neither COLLISION nor MARGIN left), RESOLVE_FAILED (status outside {0, 1}:
 *   p keeps its adopted result and is retired).  Problems that were never candidates are never written. */
#define HTP_REPAIR_MAX_ROUNDS 8
enum {                               /* int32 state[batch] */
  HTP_REPAIR_CANDIDATE = 1,          /* was selected at least once */
  HTP_REPAIR_IMPROVED = 2,           /* a re-solve was adopted */
  HTP_REPAIR_REPAIRED = 4,           /* the adopted result is clean against the original margin */
  HTP_REPAIR_RESOLVE_FAILED = 8,     /* a re-solve ended outside {0, 1}; retired */
  HTP_REPAIR_GAVE_UP = 16            /* the next margin would exceed dmin_orig + max_raise; retired */
};
typedef struct {
  int32_t rounds;                    /* 1..HTP_REPAIR_MAX_ROUNDS (pack and merge do not read it) */
  double pad;                        /* >= 0, added to every raise */
  double max_raise;                  /* > 0 */
  htp_obca_audit_opts audit;         /* of every audit the loop makes (pack and merge do not read it) */
} htp_obca_repair_opts;              /* defaults of the bindings: 3 rounds, pad 0.01 m, max_raise 0.5 m */
typedef struct {
  int32_t* state;                    /* [batch] HTP_REPAIR_* bits */
  int32_t* rounds_used;              /* [batch] re-solves merged */
  int32_t* extra_iterations;         /* [batch] their IPM iterations, adopted or not */
  double* dmin_used;                 /* [batch] the margin of the last re-solve merged */
} htp_obca_repair_state;
typedef struct {
  int32_t cap;                       /* slots of storage, >= 1 */
  int32_t* count;                    /* [1] candidates packed (may exceed cap) */
  int32_t* index;                    /* [cap] */
  int32_t* adopted;                  /* [cap] written by merge */
  double *traj, *obs_A, *obs_b, *body_G, *body_g, *params, *params_audit;   /* [cap][..] as in htp_obca_batch */
  double *init_control, *init_mu, *init_lambda;
} htp_obca_repair_slots;
typedef struct {
  htp_obca_repair_state state;
  int32_t* round_counts;             /* [HTP_REPAIR_MAX_ROUNDS][3]: selected, adopted, clean; rounds not run: 0 */
} htp_obca_repair_report;
/* API errors (-1 with a "[repair]" message, nothing launched): a null required argument (out->n_resto,
 * stage_clearance and tally may be null), N < 2 or > HTP_AUDIT_MAX_N, an edge count outside 3..8, cap < 1, pad
 * not >= 0, max_raise not > 0, rounds outside 1..HTP_REPAIR_MAX_ROUNDS, audit options the audit rejects.
 * batch == 0 returns 0.  The host variants are synchronous; the device variants are enqueued on `stream`. */
int htp_obca_repair_pack_batch(htp_ctx* ctx, const htp_obca_batch* in, const htp_obca_result* out,
                               const htp_obca_audit_result* audit, const htp_obca_repair_opts* opts,
                               htp_obca_repair_state* state, htp_obca_repair_slots* slots);
int htp_obca_repair_pack_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const htp_obca_result* out,
                                      const htp_obca_audit_result* audit, const htp_obca_repair_opts* opts,
                                      htp_obca_repair_state* state, htp_obca_repair_slots* slots, void* stream);
/* tally: nullable [3], incremented by the slots merged, adopted and clean */
int htp_obca_repair_merge_batch(htp_ctx* ctx, const htp_obca_batch* in, const htp_obca_repair_slots* slots,
                                const htp_obca_result* re, const htp_obca_audit_result* re_audit,
                                htp_obca_result* out, htp_obca_audit_result* audit, htp_obca_repair_state* state,
                                int32_t* tally);
int htp_obca_repair_merge_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const htp_obca_repair_slots* slots,
                                       const htp_obca_result* re, const htp_obca_audit_result* re_audit,
                                       htp_obca_result* out, htp_obca_audit_result* audit,
                                       htp_obca_repair_state* state, int32_t* tally, void* stream);
/* The loop: audits out->x into audit_out, then up to opts->rounds times: pack (into a workspace the library owns,
 * sized by the count), htp_obca_solve_batch_device, htp_obca_audit_batch_device against params_audit, merge; it
 * stops early when nothing is packed.  `out` is updated in place, audit_out ends as the audit of the adopted
 * results, report->state starts fresh.  The device variant runs on `stream` and reads back 4 bytes (count) per
 * round, because the solve entry takes its batch size on the host: it synchronises the stream once per round and
 * returns with the last merge enqueued.  in->init_* are not read.  Overwrites htp_last_kernel_ms (the last
 * re-solve) and htp_obca_audit_last_ms. */
int htp_obca_repair_batch(htp_ctx* ctx, const htp_obca_batch* in, htp_obca_result* out,
                          const htp_obca_repair_opts* opts, htp_obca_audit_result* audit_out,
                          htp_obca_repair_report* report);
int htp_obca_repair_batch_device(htp_ctx* ctx, const htp_obca_batch* in, htp_obca_result* out,
                                 const htp_obca_repair_opts* opts, htp_obca_audit_result* audit_out,
                                 htp_obca_repair_report* report, void* stream);
/* durations (ms) of the last pack (scan + gather kernels) and the last merge (decide + scatter kernels) */
int htp_obca_repair_last_ms(htp_ctx* ctx, double* pack_ms, double* merge_ms);

/* ---------------------------------------------------------------------------
 * Swept-footprint envelope of solved OBCA trajectories (the reference asks this of warm starts only:
 * R/car_model.py:39-73 get_path_poly unions the body and implement rectangles over a path, and
 * orchard_environment_OBCA fixes the headland's width; nothing there measures the optimised trajectory).  For
 * every problem of a batch: the extent of the placed body polygons over the densely sampled trajectory in a
 * caller-given frame, which pose and body attain it, and an occupancy raster of the swept region.
 *   Poses: exactly the audit's.  The N nodes and, with substeps = S, S - 1 poses inside every interval, from
 *   step(X_i, U_i, wheelbase, h_i q / S, time_opt), q = 1..S-1, h_i = dT tau_i (dT without time_opt): the NLP's
 *   own integrator (midpoint rule with time_opt, Euler otherwise).  The last node starts no interval.  sin, cos
 *   and tan are the planner libm's; no product and sum are contracted.
 *   Bodies: the K polygons of body_G / body_g, by the audit's construction: every row's line is clipped
 *   against the other rows of its polygon; an edge record is the unit normal (nx, ny), the offset bb, the start
 *   point and the length; a redundant row is dropped; the start points of the surviving edges are the polygon's
 *   vertices (vx, vy).  A body that is empty or unbounded is a bad polytope.  Obstacles are not read.
 *   Frame: frame[batch][3] = (ox, oy, phi), (c_phi, s_phi) = the libm's sincos(phi).  A world point w has the
 *   frame coordinates u = c_phi (wx - ox) + s_phi (wy - oy), v = c_phi (wy - oy) - s_phi (wx - ox).  For a
 *   headland, u runs along the boundary and v into the headland; the library attaches no further meaning.
 *   Extent: extent[batch][4] = (umin, umax, vmin, vmax) over every vertex of every body at every pose
 *   (x, y, c = cos theta, s = sin theta): the world vertex is (x + (c vx - s vy), y + (s vx + c vy)).
 *   where[batch][4][3] = the (stage, substep, body) that attains each of the four; ties go to the lowest
 *   flattened index (stage S + substep) K + body.  extent_body (nullable) [batch][K][4]: the same per body.
 *   Raster: W x H cells of side res anchored at the frame's origin, W a multiple of 32, W H <= 65 536.  Cell
 *   (i, j) has the centre a = (i + 0.5) res, b = (j + 0.5) res, in the world
 *   w = (ox + (c_phi a - s_phi b), oy + (s_phi a + c_phi b)), and in the body frame of a pose
 *   q = (c dx + s dy, c dy - s dx) with (dx, dy) = w - (x, y).  Body k at a pose covers the cell iff
 *   nx qx + ny qy - bb <= 0 for every surviving edge record of k.  A cell is occupied by body k iff some pose
 *   covers it, and occupied iff some body occupies it.
 *   cells[batch][K + 1]: occupied cells per body and, at index K, of the union.  bitmap (nullable) uint32
 *   [batch][H][W / 32]: the union; bit b of word w in row j is cell (32 w + b, j).  Area = cells res^2 is the
 *   caller's arithmetic.  W = H = 0 asks for the extent only: no raster work, cells and bitmap are not written,
 *   res is not read.
 *   `in` is the struct the solve took; only X, U and tau of x, the body rows, the frame and the dT and
 *   wheelbase parameters are read, so a failed solve still gets an answer.  One wavefront per problem, one
 *   launch.  The device equals a serial evaluation bit for bit: every quantity is a min / max with an index,
 *   a bit OR or a population count. */
#define HTP_ENVELOPE_MAX_N HTP_AUDIT_MAX_N   /* the LDS staging holds the audit's horizon beside a full grid */
#define HTP_ENVELOPE_MAX_CELLS 65536
enum {                               /* int32 flags[batch] */
  HTP_ENVELOPE_CLIPPED = 1,          /* umin < 0, vmin < 0, umax > W res or vmax > H res: the counts and the bitmap
                                        are of the part inside the grid (never set without a raster) */
  HTP_ENVELOPE_NONFINITE = 2,        /* a non-finite double among those read, the frame included: extent NaN, where -1,
                                        cells 0, bitmap zeroed, no other flag */
  HTP_ENVELOPE_BAD_POLYTOPE = 4      /* a body that is empty or unbounded: the same outputs */
};
typedef struct {
  int32_t substeps;                  /* 1 (nodes only) .. HTP_AUDIT_MAX_SUBSTEPS */
  double res;                        /* cell side, finite and > 0 (not read when W = H = 0) */
  int32_t W, H;                      /* cells along u and v; both 0: extent only */
} htp_obca_envelope_opts;
typedef struct {
  double* extent;           /* [batch][4] umin, umax, vmin, vmax */
  int32_t* where;           /* [batch][4][3] stage, substep, body of each */
  double* extent_body;      /* nullable [batch][K][4] */
  int32_t* cells;           /* [batch][K + 1]; may be null when W = H = 0 */
  uint32_t* bitmap;         /* nullable [batch][H][W / 32] */
  int32_t* flags;           /* [batch] HTP_ENVELOPE_* bits */
} htp_obca_envelope_result;
/* API errors (-1 with an "[envelope]" message, nothing launched): a null required argument, N < 2 or
 * > HTP_ENVELOPE_MAX_N, substeps outside 1..HTP_AUDIT_MAX_SUBSTEPS, an edge count outside 3..8, res not finite
 * or <= 0 when a raster is asked for, W not a multiple of 32, W H > HTP_ENVELOPE_MAX_CELLS, exactly one of W, H
 * being 0.  batch == 0 returns 0. */
/* host pointers, synchronous; only [X | U | tau] of every x row is uploaded */
int htp_obca_envelope_batch(htp_ctx* ctx, const htp_obca_batch* in, const double* x, const double* frame,
                            const htp_obca_envelope_opts* opts, htp_obca_envelope_result* out);
/* device pointers, enqueued on `stream`, not synchronised: behind htp_obca_solve_batch_device (and the audit) on
 * the same stream it measures that solve's out->x without a host round trip */
int htp_obca_envelope_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const double* x, const double* frame,
                                   const htp_obca_envelope_opts* opts, htp_obca_envelope_result* out, void* stream);
/* duration (ms) of the last envelope kernel (hipEvents on its stream) */
double htp_obca_envelope_last_ms(htp_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Closed-loop tracking rollout of solved OBCA trajectories (no reference counterpart: the reference plans a turn
 * and stops there).  For every problem of a batch and every one of R disturbance scenarios shared by the batch, a
 * kinematic plant is driven along the solved trajectory by a fixed tracking controller with the NLP's own actuator
 * limits, and the clearance of the placed bodies against the obstacles is measured at every control tick.
 *   Read: X, U and tau of x; the four polygon arrays; params DT, WHEELBASE (L), MAXSTEER, MAXV, MAXACC, MAXSR (their
 *   absolute values are the limits) and DMIN; the scenario table.  sin, cos, tan, atan2 and hypot are the planner
 *   libm's; no product and sum are contracted.  clamp(u, +-m) = u < -m ? -m : (u > m ? m : u); it BITES when it
 *   changes u.
 *   Reference signal.  Node times t_i and T exactly as the timeline's (serial sums of h_i = dT tau_i, dT without
 *   time_opt).  n = the smallest n with fl(n dt) >= T.  ref(k) for k < n is the timeline's regular row at
 *   s_k = fl(k dt): step(X_i, U_i, L, s_k - t_i, time_opt) with i the largest i in 0..N-2 with t_i <= s_k; ref(k)
 *   for k >= n is the stored node X_{N-1}.  Its five doubles are (xr, yr, vr, thr, dr).  Poses k = 0..n are
 *   rolled; with n + 1 > max_ticks only the first max_ticks, and every scenario gets TRUNCATED.  np = the number
 *   of poses rolled.
 *   Problem-level rejections, as the timeline's: a non-finite double among those read from x, the polygons and
 *   params -> NONFINITE; some h_i not > 0 or T / dt >= 2^30 -> BAD_TIME.  Then every scenario of the problem gets
 *   metrics NaN, worst -1 and flags = that one bit; tally counts R under that bit; worst_scenario = -1;
 *   tick_clearance and reference are not written.
 *   Scenario row (lat0, lon0, yaw0, steer_bias, slip, yaw_gain).  A row with a non-finite double: metrics NaN,
 *   worst -1, flags = NONFINITE alone; it takes no part in anything else.  Initial state, with (c0, s0) =
 *   sincos(X_0.theta):  x = (X_0.x + lon0 c0) - lat0 s0,  y = (X_0.y + lon0 s0) + lat0 c0,  v = X_0.v,
 *   theta = X_0.theta + yaw0,  delta = X_0.steer.
 *   At pose k, with (c, s) = sincos(thr) of ref(k):
 *     e_lon = c (x - xr) + s (y - yr),  e_lat = c (y - yr) - s (x - xr),  d = theta - thr,
 *     e_th = atan2(sin d, cos d);
 *     clearance_k = min over obstacles m and bodies b of the audit's signed_distance at (x, y, cos theta, sin theta),
 *     over the audit's edge records; the running minimum keeps (k, m, b), ties to the lowest (k M + m) K + b.  An
 *     empty or unbounded polygon (BAD_POLYTOPE, the audit's rule) makes the clearance metric NaN and worst -1 for
 *     every scenario of the problem; everything else is still computed;
 *     the maxima of |e_lat|, |e_lon|, |e_th| and |delta - dr| are updated; end position error = hypot(e_lon, e_lat)
 *     and end |e_th| are those of the last pose the scenario reached;
 *     if not hypot(e_lon, e_lat) <= abort_dist: DIVERGED, and the scenario stops at this pose (included).
 *   Control for tick k -> k + 1 (only while k + 1 < np), r+ = ref(k + 1), g = -1 if vr+ < 0, else +1:
 *     v_des = clamp(vr+ - k_lon e_lon, +-MAXV)               (a set-point limit: it sets no flag)
 *     a     = clamp((v_des - v) / dt, +-MAXACC)               bites -> SAT_ACC
 *     d_des = clamp((dr+ - k_lat e_lat) - (g k_yaw) e_th, +-MAXSTEER)   bites -> SAT_STEER
 *     w     = clamp((d_des - delta) / dt, +-MAXSR)            bites -> SAT_RATE
 *     Why these signs.  Near the reference e_lat' = v e_th and e_th' = v (delta - dr) / L, so with
 *     delta - dr = -k_lat e_lat - g k_yaw e_th and g = sign(v) the error dynamics are
 *       [e_lat; e_th]' = [[0, v], [-v k_lat / L, -|v| k_yaw / L]] [e_lat; e_th]:
 *     trace -|v| k_yaw / L < 0 and determinant v^2 k_lat / L > 0 in both gears, i.e. stable, with natural frequency
 *     |v| sqrt(k_lat / L) and damping ratio k_yaw / (2 sqrt(k_lat L)).  Without g the yaw term would feed back
 *     positively in reverse.
 *   Plant for tick k -> k + 1: P = plant_substeps midpoint-rule steps of hp = dt / P with a and w held:
 *     F(q) = the audit's kin at (x, y, (1 - slip) v, theta, delta + steer_bias) with controls (a, w), its heading
 *     component multiplied by yaw_gain;  q_mid = q + (0.5 hp) F(q);  q <- q + hp F(q_mid).
 *     The midpoint rule is used whatever the NLP's discretisation: the plant is the truth model.  After the P steps
 *     delta = clamp(delta, +-MAXSTEER) (it guards rounding and sets no flag).
 *   The plant is kinematic: no tyre dynamics, no actuator lag beyond the rate limit, no sensor noise; slip and
 *   yaw_gain are two constant factors.  A clear rollout is evidence, not a guarantee.
 *   One wavefront per problem, one lane per scenario, one launch.  The device equals a serial evaluation bit for
 *   bit: every lane's rollout is serial, and everything across lanes is a min with an index or a count. */
#define HTP_TRACK_MAX_N HTP_AUDIT_MAX_N
#define HTP_TRACK_NDIST 6            /* lat0, lon0, yaw0, steer_bias, slip, yaw_gain */
#define HTP_TRACK_MAX_SCENARIOS 4096
#define HTP_TRACK_MAX_SUBSTEPS 16
#define HTP_TRACK_NREF 5             /* xr, yr, vr, thr, dr */
enum {                               /* double metrics[batch][R][HTP_TRACK_NMETRIC] */
  HTP_TRACK_CLEARANCE = 0,           /* min clearance over the poses reached */
  HTP_TRACK_MAX_ELAT,                /* max |e_lat| */
  HTP_TRACK_MAX_ELON,                /* max |e_lon| */
  HTP_TRACK_MAX_ETH,                 /* max |e_th| */
  HTP_TRACK_END_POS,                 /* hypot(e_lon, e_lat) at the last pose reached */
  HTP_TRACK_END_ETH,                 /* |e_th| at the last pose reached */
  HTP_TRACK_MAX_STEER_DEV,           /* max |delta - dr| */
  HTP_TRACK_SAT_SHARE,               /* control ticks with a biting a, d_des or w clamp / control ticks taken; 0 if none */
  HTP_TRACK_NMETRIC
};
enum {                               /* int32 flags[batch][R]; bit b is tally column b */
  HTP_TRACK_COLLISION = 1,           /* clearance < 0 */
  HTP_TRACK_MARGIN = 2,              /* clearance < params[HTP_P_DMIN] - margin_tol */
  HTP_TRACK_SAT_STEER = 4,
  HTP_TRACK_SAT_RATE = 8,
  HTP_TRACK_SAT_ACC = 16,
  HTP_TRACK_DIVERGED = 32,
  HTP_TRACK_TRUNCATED = 64,
  HTP_TRACK_NONFINITE = 128,
  HTP_TRACK_BAD_POLYTOPE = 256,
  HTP_TRACK_BAD_TIME = 512
};
#define HTP_TRACK_NFLAG 10
typedef struct {
  double dt;                         /* control period, finite and > 0 */
  int32_t max_ticks;                 /* poses of storage per problem, >= 2 */
  int32_t plant_substeps;            /* 1 .. HTP_TRACK_MAX_SUBSTEPS */
  double k_lat, k_yaw, k_lon;        /* finite and >= 0 */
  double abort_dist;                 /* > 0 (may be infinite) */
  double margin_tol;                 /* finite and >= 0 */
  int32_t R;                         /* scenarios, 1 .. HTP_TRACK_MAX_SCENARIOS */
  const double* scenarios;           /* [R][HTP_TRACK_NDIST], shared by the batch */
} htp_obca_track_opts;
typedef struct {
  double* metrics;          /* [batch][R][HTP_TRACK_NMETRIC] */
  int32_t* worst;           /* [batch][R][3] tick, obstacle, body of HTP_TRACK_CLEARANCE */
  int32_t* flags;           /* [batch][R] HTP_TRACK_* bits */
  int32_t* tally;           /* [batch][HTP_TRACK_NFLAG] scenarios carrying each flag */
  int32_t* worst_scenario;  /* [batch] argmin of the clearance metric over the scenarios, ties to the lowest; -1 if no
                               scenario has a clearance */
  double* tick_clearance;   /* nullable [batch][max_ticks]: per pose the min of clearance_k over the scenarios that
                               reached it (+inf if none did, NaN with BAD_POLYTOPE); entries at or beyond np are
                               never written */
  double* reference;        /* nullable [batch][max_ticks][HTP_TRACK_NREF]: ref(k), k < np; the rest never written */
} htp_obca_track_result;
/* API errors (-1 with a "[track]" message, nothing launched): a null required argument, N < 2 or > HTP_TRACK_MAX_N,
 * dt not finite or <= 0, max_ticks < 2, plant_substeps outside 1..16, R < 1 or > 4096, a negative or non-finite
 * gain or margin_tol, abort_dist not > 0, an edge count outside 3..8.  batch == 0 returns 0.  Nothing beyond the
 * batch is ever written. */
/* host pointers, synchronous; only [X | U | tau] of every x row is uploaded; the entries of tick_clearance and
 * reference that are never written keep the caller's values */
int htp_obca_track_batch(htp_ctx* ctx, const htp_obca_batch* in, const double* x, const htp_obca_track_opts* opts,
                         htp_obca_track_result* out);
/* device pointers (opts->scenarios too), enqueued on `stream`, not synchronised: behind htp_obca_solve_batch_device
 * (and the audit or the repair) on the same stream it rolls that solve's out->x without a host round trip */
int htp_obca_track_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const double* x,
                                const htp_obca_track_opts* opts, htp_obca_track_result* out, void* stream);
/* duration (ms) of the last track kernel (hipEvents on its stream) */
double htp_obca_track_last_ms(htp_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Time-varying LQR gains and error tube of solved OBCA trajectories (no reference counterpart: the reference returns
 * a trajectory and no controller for it).  For every problem of a batch: the NLP's own integrator linearised at
 * every stage, the finite-horizon LQR gains K_i about the solved trajectory, the one-sigma tube of the tracking
 * error and of the feedback's control effort under that law, and the authority the limits leave beside the
 * reference.  Everything is a function of X, U and tau of x, six parameters and the options alone.
 *   Read: X, U and tau of x; params DT, WHEELBASE (L), MAXSTEER, MAXV, MAXACC, MAXSR (as they stand, no absolute
 *   value).  Polygons and duals are never read (the polygon arrays of `in` may be null).  sin, cos and tan are the
 *   planner libm's; no product and sum are contracted.
 *   State s = (x, y, v, theta, delta), control u = (a, w), f = the audit's kin =
 *   (v cos theta, v sin theta, a, v tan delta / L, w); h_i = dT tau_i with time_opt, else dT; i = 0..N-2.
 *   Jacobians.  Fx(s) has the entries (row, column)
 *     (x, v) = cos theta          (x, theta) = -v sin theta
 *     (y, v) = sin theta          (y, theta) = v cos theta
 *     (theta, v) = tan delta / L  (theta, delta) = v / (L (cos delta)^2)
 *   and zeros elsewhere; Fu has (v, a) = 1 and (delta, w) = 1.
 *   Linearisation of the integrator about (X_i, U_i, h = h_i):
 *     Euler (no time_opt):  A_i = I + h Fx(X_i),  B_i = h Fu.
 *     Midpoint (time_opt):  m = X_i + (h / 2) f(X_i, U_i),  A_i = I + h Fx(m) (I + (h / 2) Fx(X_i)),
 *                           B_i = h (Fu + (h / 2) Fx(m) Fu).
 *   Products with the structural zeros and ones are not formed: rows v and delta of A_i are unit rows, columns x
 *   and y unit columns, (theta, theta) is 1; B_i has (v, a) = (delta, w) = h, with time_opt also (x, a), (y, a),
 *   (theta, a) and (theta, w), and zeros elsewhere.  With F = Fx(X_i), G = Fx(m) and hh = h / 2 the free entries are
 *     A(r, v) = h (G(r, v) + G(r, theta) (hh F(theta, v))),  A(r, theta) = h G(r, theta),
 *     A(r, delta) = h (G(r, theta) (hh F(theta, delta)))               for r = x, y;
 *     A(theta, v) = h G(theta, v),  A(theta, delta) = h G(theta, delta);
 *     B(r, a) = h (hh G(r, v)) for r = x, y, theta,  B(theta, w) = h (hh G(theta, delta)).
 *   Weights (options, shared by the batch).  Q_i is diag(q_lon, q_lat, q_v, q_th, q_st) in the frame of node i, in
 *   world coordinates with c = cos theta_i, s = sin theta_i:
 *     Qxx = (c c) q_lon + (s s) q_lat,  Qxy = Qyx = (c s) (q_lon - q_lat),  Qyy = (s s) q_lon + (c c) q_lat,
 *   the rest diagonal.  R = diag(r_a / MAXACC^2, r_w / MAXSR^2): the weights are on the controls normalised by the
 *   problem's own limits, so one table suits a batch with different limits.
 *   Backward pass.  P_{N-1} = qf Q_{N-1}.  For i = N-2 down to 0, with P = P_{i+1}, A = A_i, B = B_i:
 *     T = P A,  S = R + B' (P B) (2 x 2),  K_i = S^-1 (B' T) by the closed-form inverse:
 *       det = S00 S11 - S01 S10,  K(0, c) = (S11 g0 - S01 g1) / det,  K(1, c) = (S00 g1 - S10 g0) / det
 *       with (g0, g1) = column c of B' T;
 *     P_i = Q_i + T' (A - B K_i)   (= Q_i + A' P (A - B K_i): P is symmetric bit for bit),  then
 *     P_i <- (P_i + P_i') / 2.
 *   Every inner product is summed over k = 0..4 from left to right, the products with the structural zeros and
 *   ones included; (B K)(r, c) = B(r, a) K(a, c) + B(r, w) K(w, c).
 *   The feedback law is u = U_i - K_i (s - X_i); wrapping the theta difference of (s - X_i) is the caller's.
 *   Forward pass.  Sigma_0 = diag(sig0_lon^2, sig0_lat^2, sig0_v^2, sig0_th^2, sig0_st^2) in the frame of X_0, in
 *   world coordinates as Q.  With Acl = A_i - B_i K_i:
 *     Sigma_{i+1} = (Acl Sigma_i) Acl' + h_i W_i,  then symmetrised as P;
 *   W_i = diag(w_lon, w_lat, w_v, w_th, w_st) (variance per second) in the frame of node i, in world coordinates.
 *   Tube row of node i, with c, s of theta_i and Sigma = Sigma_i:
 *     var_lon = c (c Sxx + s Sxy) + s (c Syx + s Syy),  var_lat = s (s Sxx - c Sxy) - c (s Syx - c Syy),
 *     var_v, var_theta, var_delta = the diagonal,  var_a, var_w = diag((K_i Sigma) K_i')  (0 at node N-1);
 *     the row is the square roots (sigma_lon, sigma_lat, sigma_v, sigma_theta, sigma_delta, sigma_a, sigma_w); a
 *     negative radicand is 0.
 *   Authority.  Headroom: MAXACC - |a_i| and MAXSR - |w_i| at the stages i = 0..N-2, MAXSTEER - |delta_i| and
 *   MAXV - |v_i| at the nodes i = 0..N-1.  ratio = headroom / sigma of the same quantity (sigma_a, sigma_w,
 *   sigma_delta, sigma_v); +inf where sigma = 0 and headroom >= 0; negative where the reference itself is beyond
 *   the limit.  The metrics carry each ratio's minimum over its stages.
 *   Rejections: a non-finite double among those read -> NONFINITE; some h_i not > 0 -> BAD_TIME; a limit or the
 *   wheelbase not > 0 -> BAD_LIMIT (both bits where both hold).  Then metrics are NaN, flags is those bits, and
 *   nothing else is written.
 *   SINGULAR.  Backward, at stage i: det not > 0, or a non-finite det, K_i or P_i entry.  Then the rows 0..i of
 *   gains and of cost_to_go are NaN (the rows above keep their values), every tube row and every metric is NaN,
 *   worst is -1; linearisation is complete.  Forward, at node i: a non-finite entry of the tube row or of
 *   Sigma_{i+1}.  Then the tube rows i..N-1 and every metric are NaN and worst is -1.  No other flag is set.
 *   The model is linear and the noise Gaussian and white; the clamps of the actuators are ignored, and the ratios
 *   say where that assumption breaks.  The tube is evidence, not a bound.
 *   One wavefront per problem, one launch.  The device equals a serial evaluation bit for bit: a stage's
 *   linearisation is serial, every entry of every product is one serial sum, nothing is summed across lanes. */
#define HTP_LQR_MAX_N HTP_AUDIT_MAX_N
#define HTP_LQR_NTUBE 7              /* sigma_lon, sigma_lat, sigma_v, sigma_theta, sigma_delta, sigma_a, sigma_w */
#define HTP_LQR_NGAIN 10             /* K_i row-major: 2 x 5 */
#define HTP_LQR_NCTG 15              /* upper triangle of P_i, row-major */
#define HTP_LQR_NLIN 35              /* A_i row-major (25), then B_i row-major (10) */
enum {                               /* double metrics[batch][HTP_LQR_NMETRIC] */
  HTP_LQR_MAX_SLAT = 0,              /* max sigma_lat over the nodes */
  HTP_LQR_MAX_SLON,                  /* max sigma_lon */
  HTP_LQR_MAX_STH,                   /* max sigma_theta */
  HTP_LQR_END_SLAT,                  /* sigma_lat at node N-1 */
  HTP_LQR_MAX_GAIN,                  /* max |K_i| entry over the stages */
  HTP_LQR_TRACE_P0,                  /* trace P_0 */
  HTP_LQR_RATIO_ACC,                 /* min (MAXACC - |a_i|) / sigma_a */
  HTP_LQR_RATIO_RATE,                /* min (MAXSR - |w_i|) / sigma_w */
  HTP_LQR_RATIO_STEER,               /* min (MAXSTEER - |delta_i|) / sigma_delta */
  HTP_LQR_RATIO_SPEED,               /* min (MAXV - |v_i|) / sigma_v */
  HTP_LQR_NMETRIC
};
enum {                               /* int32 flags[batch] */
  HTP_LQR_AUTHORITY_ACC = 1,         /* HTP_LQR_RATIO_ACC < k_sigma */
  HTP_LQR_AUTHORITY_RATE = 2,
  HTP_LQR_AUTHORITY_STEER = 4,
  HTP_LQR_AUTHORITY_SPEED = 8,
  HTP_LQR_SINGULAR = 16,
  HTP_LQR_NONFINITE = 32,
  HTP_LQR_BAD_TIME = 64,
  HTP_LQR_BAD_LIMIT = 128
};
typedef struct {
  double q_lon, q_lat, q_v, q_th, q_st;            /* state weights, finite and >= 0 */
  double qf;                                       /* terminal factor, finite and >= 0 */
  double r_a, r_w;                                 /* control weights, finite and > 0 */
  double sig0_lon, sig0_lat, sig0_v, sig0_th, sig0_st;   /* initial standard deviations, finite and >= 0 */
  double w_lon, w_lat, w_v, w_th, w_st;            /* noise, variance per second, finite and >= 0 */
  double k_sigma;                                  /* >= 0 (may be infinite) */
} htp_obca_lqr_opts;
typedef struct {
  double* gains;            /* [batch][N-1][2][5] K_i */
  double* tube;             /* [batch][N][HTP_LQR_NTUBE] */
  double* metrics;          /* [batch][HTP_LQR_NMETRIC] */
  int32_t* worst;           /* [batch][2] the node of HTP_LQR_MAX_SLAT and the stage of HTP_LQR_RATIO_RATE; ties go
                               to the lowest */
  int32_t* flags;           /* [batch] HTP_LQR_* bits */
  double* cost_to_go;       /* nullable [batch][N][HTP_LQR_NCTG] */
  double* linearisation;    /* nullable [batch][N-1][HTP_LQR_NLIN] */
} htp_obca_lqr_result;
/* API errors (-1 with an "[lqr]" message, nothing launched): a null required argument, N < 2 or > HTP_LQR_MAX_N,
 * a negative or non-finite weight or sigma, r_a or r_w not > 0, k_sigma not >= 0, M, K or an edge count outside
 * their ranges (3..8 for an edge count; they set the stride of x).  batch == 0 returns 0.  Nothing beyond the
 * batch is ever written. */
/* host pointers, synchronous; only [X | U | tau] of every x row is uploaded; what a flag leaves unwritten keeps the
 * caller's values */
int htp_obca_lqr_batch(htp_ctx* ctx, const htp_obca_batch* in, const double* x, const htp_obca_lqr_opts* opts,
                       htp_obca_lqr_result* out);
/* device pointers, enqueued on `stream`, not synchronised: behind htp_obca_solve_batch_device on the same stream it
 * reads that solve's out->x without a host round trip */
int htp_obca_lqr_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const double* x, const htp_obca_lqr_opts* opts,
                              htp_obca_lqr_result* out, void* stream);
/* duration (ms) of the last lqr kernel (hipEvents on its stream) */
double htp_obca_lqr_last_ms(htp_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Closed-loop rollout of solved OBCA trajectories under their time-varying LQR gains (no reference counterpart).
 * The tracking rollout above with one change: the fixed three-gain controller is replaced by the law
 * u = u_ff - K_i e of the LQR section, with the gains K_i handed in (htp_obca_lqr_result.gains of the same x).
 *   Exactly as the tracking rollout's text above, word for word: what is read (plus the gains); node times, n, np and
 *   TRUNCATED; ref(k); the problem-level rejections; the scenario row and the initial state; the errors, the
 *   clearance and the maxima at pose k; DIVERGED; the plant; BAD_POLYTOPE; the tally; the worst scenario.  The eight
 *   metrics and the ten flag bits are HTP_TRACK_*.
 *   Gains.  All 10 (N - 1) gains of a problem count as read: a non-finite one is the problem-level NONFINITE
 *   rejection (so a problem the LQR left SINGULAR, whose gain rows are NaN, is rejected).
 *   Control for tick k -> k + 1 (only while k + 1 < np).  i = the largest index in 0..N-2 with t_i <= fl(k dt) (the
 *   interval rule of ref(k), applied for k >= n too), (ci, si) = sincos(X_i.theta), K = K_i (2 x 5, rows a and w,
 *   columns x, y, v, theta, delta).  For r = 0 (a) and r = 1 (w):
 *     k_lon(r) = ci K(r,0) + si K(r,1),   k_lat(r) = ci K(r,1) - si K(r,0)
 *   i.e. the position gains rotated into the frame of node i; they are applied to the errors taken in the frame of
 *   ref(k): with ref(k) = X_i this is K_i (s - X_i) algebraically, inside a stage the law follows the heading of the
 *   reference.  With (xr, yr, vr, thr, dr) = ref(k), e_lon, e_lat and e_th those of pose k (the wrapped atan2 is
 *   the wrapping the LQR text leaves to the caller), e_v = v - vr and e_d = delta - dr:
 *     fb(r) = (((k_lon(r) e_lon + k_lat(r) e_lat) + K(r,2) e_v) + K(r,3) e_th) + K(r,4) e_d
 *   Feedforward, r+ = ref(k + 1):  a_ff = (vr+ - vr) / dt,  w_ff = (dr+ - dr) / dt.  Both of the NLP's integrators
 *   are linear in a and w for v and delta, so this is the tick's mean control even where the tick straddles a stage
 *   boundary (holding U_i would not be).
 *     a_cmd = a_ff - fb(0),   w_cmd = w_ff - fb(1)
 *     v_des = clamp(v + dt a_cmd, +-MAXV)                    (a set-point limit: it sets no flag)
 *     a     = clamp((v_des - v) / dt, +-MAXACC)               bites -> SAT_ACC
 *     d_des = clamp(delta + dt w_cmd, +-MAXSTEER)             bites -> SAT_STEER
 *     w     = clamp((d_des - delta) / dt, +-MAXSR)            bites -> SAT_RATE
 *   SAT_SHARE counts ticks as the tracking rollout does.
 *   tick_error[k] = the maxima over the scenarios that reached pose k of (|e_lat|, |e_lon|, |e_th|), in that order;
 *   0 where none did; an error that is NaN counts as 0.  A maximum does not depend on the order it is taken in.  It
 *   is not written for a rejected problem, nor at or beyond np.
 *   What it does not promise.  K_i was designed for the step h_i and is applied at the period dt; the clamps are
 *   outside the design; the plant's slip, bias and yaw gain are outside the LQR's noise model.  Whether the law
 *   helps is a question to measure (tools/ltrack_outcomes.py), not a property of this entry.
 *   One wavefront per problem, one lane per scenario, one launch; the device equals a serial evaluation bit for
 *   bit, as the tracking rollout does. */
typedef struct {
  double dt;                         /* control period, finite and > 0 */
  int32_t max_ticks;                 /* poses of storage per problem, >= 2 */
  int32_t plant_substeps;            /* 1 .. HTP_TRACK_MAX_SUBSTEPS */
  double abort_dist;                 /* > 0 (may be infinite) */
  double margin_tol;                 /* finite and >= 0 */
  int32_t R;                         /* scenarios, 1 .. HTP_TRACK_MAX_SCENARIOS */
  const double* scenarios;           /* [R][HTP_TRACK_NDIST], shared by the batch */
  const double* gains;               /* [batch][N-1][2][5], the layout of htp_obca_lqr_result.gains */
} htp_obca_ltrack_opts;
typedef struct {
  double* metrics;          /* [batch][R][HTP_TRACK_NMETRIC] */
  int32_t* worst;           /* [batch][R][3] */
  int32_t* flags;           /* [batch][R] HTP_TRACK_* bits */
  int32_t* tally;           /* [batch][HTP_TRACK_NFLAG] */
  int32_t* worst_scenario;  /* [batch] */
  double* tick_clearance;   /* nullable [batch][max_ticks] */
  double* reference;        /* nullable [batch][max_ticks][HTP_TRACK_NREF] */
  double* tick_error;       /* nullable [batch][max_ticks][3]: max |e_lat|, |e_lon|, |e_th| per pose; entries at or
                               beyond np are never written */
} htp_obca_ltrack_result;
/* API errors (-1 with an "[ltrack]" message, nothing launched): those of the tracking rollout less its gain checks,
 * and a null gains.  batch == 0 returns 0.  Nothing beyond the batch is ever written. */
/* host pointers (scenarios and gains too), synchronous; the entries of the three per-tick outputs that are never
 * written keep the caller's values */
int htp_obca_ltrack_batch(htp_ctx* ctx, const htp_obca_batch* in, const double* x, const htp_obca_ltrack_opts* opts,
                          htp_obca_ltrack_result* out);
/* device pointers (scenarios and gains too), enqueued on `stream`, not synchronised: behind
 * htp_obca_solve_batch_device and htp_obca_lqr_batch_device on the same stream it rolls that solve's out->x under
 * that pass's out->gains without a host round trip */
int htp_obca_ltrack_batch_device(htp_ctx* ctx, const htp_obca_batch* in, const double* x,
                                 const htp_obca_ltrack_opts* opts, htp_obca_ltrack_result* out, void* stream);
/* duration (ms) of the last ltrack kernel (hipEvents on its stream) */
double htp_obca_ltrack_last_ms(htp_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Warm start -> OBCA initial guess (R/obca_py/util.py get_init_ref_path :62-113
 * with cubic_spline.calc_spline_course :92-112): split at gear changes,
 * re-spline every segment over arc length at ds, v = gear * desired_v,
 * steer = atan(L kappa) (sign-flipped in reverse), headings unwrapped,
 * v = 0 at both ends.  One path per wavefront.  Only xs, ys and dirs are read
 * (the reference ignores the yaw and curvature columns). */
enum { HTP_RP_OK = 0, HTP_RP_OVERFLOW = 1 /* n_rows = rows needed so far */, HTP_RP_BAD_SEGMENT = 2,
       HTP_RP_BAD_INPUT = 3 };
typedef struct {
  int32_t batch, cap_points, cap_rows;  /* cap_points >= points of every path                  */
  const int32_t* path_off;              /* [batch+1] CSR offsets into xs / ys / dirs           */
  const double* xs;
  const double* ys;
  const double* dirs;                   /* +1 forward, -1 reverse                              */
  const double* params;                 /* [batch][3]: WHEEL_BASE, desired_v, ds               */
} htp_refpath_batch;
typedef struct {
  int32_t* status;                      /* [batch] HTP_RP_*                                    */
  int32_t* n_rows;                      /* [batch]                                             */
  double* traj;                         /* [batch][cap_rows][5] x, y, v, theta, steer          */
} htp_refpath_result;
int htp_init_ref_path_batch(htp_ctx* ctx, const htp_refpath_batch* in, htp_refpath_result* out);
int htp_init_ref_path_batch_device(htp_ctx* ctx, const htp_refpath_batch* in, htp_refpath_result* out, void* stream);
double htp_init_ref_path_last_ms(htp_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Reeds-Shepp: all admissible paths between pose pairs, sampled
 * (R/path_planner/utils/reeds_shepp.py calc_all_paths :39-65, called by
 * hybrid_a_star_search.py:248 and safety_forward_path_plan.py:368).
 * Query q = (sx, sy, syaw, gx, gy, gyaw, maxc, step_size).  Output is CSR:
 * paths of query q are [path_offsets[q], path_offsets[q+1]); samples of path p
 * are [point_offsets[p], point_offsets[p+1]).  Path order, lengths, ctypes,
 * sample count and values follow the reference (de-duplication, MAX_LENGTH
 * filter and trailing-zero pop included). */
enum { HTP_RS_SEG_L = 0, HTP_RS_SEG_S = 1, HTP_RS_SEG_R = 2, HTP_RS_SEG_NONE = 3 };
enum {
  HTP_RS_OK = 0,
  HTP_RS_ASSERT = 1,      /* reference raises AssertionError (a path with L < 0.01); no paths returned */
  HTP_RS_OVERFLOW = 2,    /* reference raises IndexError in generate_local_course; no paths returned */
  HTP_RS_CAPACITY = 3     /* return code only: output capacity too small, totals reported */
};

typedef struct {
  int64_t cap_paths, cap_points;  /* in: capacity of the arrays below */
  int64_t n_paths, n_points;      /* out: totals needed/written */
  int64_t* path_offsets;          /* [batch+1] */
  int32_t* status;                /* [batch] HTP_RS_* */
  double* lengths;                /* [cap_paths][5] PATH.lengths (unused entries 0) */
  int8_t* ctypes;                 /* [cap_paths][5] HTP_RS_SEG_* */
  double* L;                      /* [cap_paths] PATH.L */
  int64_t* point_offsets;         /* [cap_paths+1] */
  double *x, *y, *yaw, *cs;       /* [cap_points] PATH.x/.y/.yaw/.cs */
  int8_t* directions;             /* [cap_points] PATH.directions */
} htp_rs_paths;

/* Host buffers (synchronous).  Returns HTP_RS_CAPACITY with n_paths/n_points
 * (and status) filled when a capacity is too small; call again with larger
 * arrays (caps 0 = size query). */
int htp_rs_all_paths_batch(htp_ctx* ctx, int32_t batch, const double* queries, htp_rs_paths* out);
/* Device buffers, enqueued on `stream`.  `totals` (device int64[2]) receives
 * (n_paths, n_points); arrays are written only where they fit the capacities
 * (points beyond cap_points and paths beyond cap_paths are skipped). */
int htp_rs_all_paths_batch_device(htp_ctx* ctx, int32_t batch, const double* queries, htp_rs_paths* out,
                                  int64_t* totals, void* stream);
/* Duration (ms) of the last RS batch (hipEvents around its kernels). */
double htp_rs_last_ms(htp_ctx* ctx);


/* ---------------------------------------------------------------------------
 * Hybrid A* warm-start search (motion_type "King": Reeds-Shepp goal shots),
 * one search per problem of the batch:
 *   HybridAStarSearch(start_pose, goal_pose, config_environment, car_model,
 *                     search_heuristic, motion_type="King", yaw_resolution,
 *                     plan_resolution).hybrid_a_star_search(max_nodes)
 *   R/path_planner/hybrid_a_star_search.py:38-74 (ctor), :497-607 (search),
 * called from R/path_planner/headland_path_planning.py:203-219 and
 * R/test/obca.ipynb:261-272.  The environment and the heuristic are lowered to
 * polygons (host side, headland_trajectory_planning_amd/path_planner):
 *   body      car_model.car_poly (car_model.py:102-120), vertices in the car frame
 *   blockers  orchard_geometry_environment.py tree_polys + obstacle_polys
 *             (check_path_feasibility :423-437)
 *   field     field_range_poly (:374-378, boundary_check=True); -1 = none
 *   lanes     reference_line_heuristic.py segment_lanes (CCW, convex) with
 *             their search_lengths (:84-96); their union is guided_lane
 *   guide     guided_path rows (x, y, yaw, s) (:50-82)
 *   motions   motion steers (steer, direction) (:331-354)
 * Polygons are vertex ranges [poly_off[p], poly_off[p+1]) of `vertices`
 * (no repeated closing vertex).  Per-search descriptor desc[b][HTP_HA_NDESC]
 * holds polygon / guide / motion index ranges into these shared pools. */
#define HTP_HA_NPARAM 16
enum {
  HTP_HA_P_SX = 0, HTP_HA_P_SY, HTP_HA_P_SYAW, HTP_HA_P_GX, HTP_HA_P_GY, HTP_HA_P_GYAW,
  HTP_HA_P_RES,      /* plan_resolution */
  HTP_HA_P_YAWRES,   /* yaw_resolution */
  HTP_HA_P_WB,       /* car_model.WHEEL_BASE */
  HTP_HA_P_MAXSTEER, /* car_model.MAX_STEER */
  HTP_HA_P_CURV,     /* car_model.curvature = tan(MAX_STEER) / WHEEL_BASE */
  HTP_HA_P_DEFLEN,   /* search_heuristic.default_search_length */
  HTP_HA_P_MAXNODES  /* max_nodes */
};
#define HTP_HA_NDESC 12
enum {
  HTP_HA_D_BODY = 0,                   /* polygon id of the body */
  HTP_HA_D_BLK0, HTP_HA_D_BLK1,        /* blocker polygon ids [BLK0, BLK1) */
  HTP_HA_D_LANE0, HTP_HA_D_LANE1,      /* lane polygon ids [LANE0, LANE1) */
  HTP_HA_D_FIELD,                      /* field polygon id or -1 */
  HTP_HA_D_GUIDE0, HTP_HA_D_GUIDE1,    /* guide rows [GUIDE0, GUIDE1) */
  HTP_HA_D_MOT0, HTP_HA_D_MOT1,        /* motion rows [MOT0, MOT1) */
  HTP_HA_D_KING                        /* 1 = King (Reeds-Shepp goal shots), 0 = Pawn (Dubins + spline) */
};
enum {
  HTP_HA_FOUND = 0,            /* goal reached (Reeds-Shepp shot or within one cell) */
  HTP_HA_NO_PATH = 1,          /* open set exhausted ("No solution is available") */
  HTP_HA_MAX_NODES = 2,        /* counter > max_nodes ("drop the planner") */
  HTP_HA_START_GOAL_BLOCKED = 3,
  HTP_HA_RS_ERROR = 4,         /* the reference raises inside reeds_shepp.calc_all_paths */
  HTP_HA_CAPACITY = 5,         /* node pool exhausted (cannot happen with the library's sizing) */
  HTP_HA_BAD_INPUT = 6,        /* a per-search shape check failed (see the limits below); the search is not run */
  HTP_HA_BACKTRACK = 7         /* the reference raises KeyError while backtracking */
};
/* Per-search limits (hastar_core.h valid_search; a search outside them ends HTP_HA_BAD_INPUT on the device and in
 * the host build alike): body polygon 3..HTP_HA_MAX_BODY vertices, at most HTP_HA_MAX_LANES lane polygons and
 * HTP_HA_MAX_MOTIONS motion primitives, and for every search length L (HTP_HA_P_DEFLEN and each lane's lane_len)
 * n = rint(L / HTP_HA_P_RES) with 1 <= n, n + 1 <= HTP_HA_MAX_POSES and nmotions * (n + 1) <= HTP_HA_TRAJ_CAP:
 * one expansion's rollouts are held in LDS.  The reference has no such limit; its planners' settings need at most
 * 14 x 16 = 224 (King, search length 1.5 m at 0.1 m).  King's 14 motions allow n + 1 <= 36 poses per primitive,
 * i.e. L <= 35 res (3.5 m at 0.1 m). */
#define HTP_HA_MAX_BODY 8
#define HTP_HA_MAX_LANES 32
#define HTP_HA_MAX_MOTIONS 16
#define HTP_HA_MAX_POSES 64
#define HTP_HA_TRAJ_CAP 512

typedef struct {
  int32_t batch;
  int32_t npoly, nvert, nguide, nmotion;  /* pool sizes */
  const double* params;     /* [batch][HTP_HA_NPARAM] */
  const int32_t* desc;      /* [batch][HTP_HA_NDESC] */
  const int32_t* poly_off;  /* [npoly+1] */
  const double* vertices;   /* [nvert][2] */
  const double* lane_len;   /* [npoly] search length of lane polygons (others unused) */
  const double* guide;      /* [nguide][4] */
  const double* motions;    /* [nmotion][2] */
  int32_t max_nodes_cap;    /* >= every params[b][HTP_HA_P_MAXNODES] (sizes the node pool) */
  int32_t cap_path;         /* samples per search in the path outputs */
  int32_t cap_log;          /* expansions per search in the expansion log (0 = none) */
} htp_hastar_batch;

typedef struct {
  int32_t* status;      /* [batch] HTP_HA_* */
  int32_t* counter;     /* [batch] the reference's returned node counter */
  int32_t* n_path;      /* [batch] samples of the returned path (may exceed cap_path: then truncated) */
  int32_t* n_expanded;  /* [batch] nodes popped */
  int64_t* n_pose;      /* [batch] footprint poses tested */
  double *x, *y, *yaw, *dir, *k;  /* [batch][cap_path]: xs, ys, yaws, dirs, ks of the search result */
  int32_t* expanded;    /* [batch][cap_log][3] grid index of every popped node (nullable) */
} htp_hastar_result;

/* Host buffers in and out (synchronous). */
int htp_hastar_search_batch(htp_ctx* ctx, const htp_hastar_batch* in, htp_hastar_result* out);
/* Device buffers in and out, enqueued on `stream`. */
int htp_hastar_search_batch_device(htp_ctx* ctx, const htp_hastar_batch* in, htp_hastar_result* out, void* stream);
/* Duration (ms) of the last search kernel (hipEvents on its stream). */
double htp_hastar_last_ms(htp_ctx* ctx);


/* ---------------------------------------------------------------------------
 * Y-type parking grid search: search_y_type_parking_path(car_model, config_env,
 * end_pose, backward_steer_dir, forward_steer_dir, max/min steers and lengths,
 * step_size) R/path_planner/headland_path_planning.py:382-451, one search per
 * problem of the batch.  The grid axes (np.arange values, the reference's loop
 * order: backward length, forward length, backward steer, forward steer) live in
 * `axis`; the first collision-free candidate is returned with its manoeuvre
 * (rows x, y, yaw, k, dir in the odom frame, get_y_type_parking_path +
 * get_path_in_odom :487-527).  Footprint = car_poly at every pose against
 * blockers (obstacle + tree polygons) and inside the field polygon
 * (check_path_feasibility :423-458, boundary_check=True). */
#define HTP_YP_NPARAM 16
enum {
  HTP_YP_P_EX = 0, HTP_YP_P_EY, HTP_YP_P_EYAW,  /* end (row-enter) pose */
  HTP_YP_P_BDIR, HTP_YP_P_FDIR,                 /* backward / forward steer directions (+-1) */
  HTP_YP_P_WB, HTP_YP_P_STEP,                   /* car_model.WHEEL_BASE, step_size */
  HTP_YP_P_R00, HTP_YP_P_R01, HTP_YP_P_R10, HTP_YP_P_R11, HTP_YP_P_TX, HTP_YP_P_TY,  /* states2SE3(end pose) */
  HTP_YP_P_YAW_ODOM                             /* SE32states(T)[5] */
};
#define HTP_YP_NDESC 12
enum {
  HTP_YP_D_BODY = 0, HTP_YP_D_BLK0, HTP_YP_D_BLK1, HTP_YP_D_FIELD,
  HTP_YP_D_BL0, HTP_YP_D_NBL, HTP_YP_D_FL0, HTP_YP_D_NFL, HTP_YP_D_SB0, HTP_YP_D_NSB, HTP_YP_D_SF0, HTP_YP_D_NSF
};
enum { HTP_YP_FOUND = 0, HTP_YP_NONE = 1, HTP_YP_END_BLOCKED = 2, HTP_YP_BAD_INPUT = 3 };

typedef struct {
  int32_t batch, npoly, nvert, naxis;
  const double* params;     /* [batch][HTP_YP_NPARAM] */
  const int32_t* desc;      /* [batch][HTP_YP_NDESC] */
  const int32_t* poly_off;  /* [npoly+1] */
  const double* vertices;   /* [nvert][2] */
  const double* axis;       /* [naxis] grid axis values */
  int32_t cap_path;         /* rows per search in `path` */
} htp_ypark_batch;

typedef struct {
  int32_t* status;   /* [batch] HTP_YP_* */
  int32_t* cand;     /* [batch] index of the chosen candidate in loop order (-1: none) */
  int32_t* n_path;   /* [batch] rows of the chosen manoeuvre */
  double* params;    /* [batch][4] backward length, forward length, backward steer, forward steer */
  int64_t* n_pose;   /* [batch] footprint poses tested (nullable) */
  double* path;      /* [batch][cap_path][5] */
} htp_ypark_result;

int htp_ypark_search_batch(htp_ctx* ctx, const htp_ypark_batch* in, htp_ypark_result* out);
int htp_ypark_search_batch_device(htp_ctx* ctx, const htp_ypark_batch* in, htp_ypark_result* out, void* stream);
double htp_ypark_last_ms(htp_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Orchard scene -> OBCA obstacles: the synthetic orchard
 * of R/path_planner/utils/map_utils.py create_tree_rows :45-61 and the OGE_OBCA
 * obstacle producer, one scene per GPU thread (csrc/oge_core.h):
 *   env = orchard_environment_OBCA(tree_rows, [], tree_width, headland_width)
 *   boundary = env.create_boundary_polygons()          OGE_OBCA.py:306-373
 *   rows = env.get_obstacle_tree_rows(start, end)      :477-591
 *   obstacles = env.get_obstacles_for_OBCA(boundary, rows, start, end, side)  :593-677
 * and, per obstacle, compute_polytope_halfspaces as R/obca_py/optimizer.py:184-186
 * calls it (A x <= b, cdd row normalisation, 7-decimal rounding).  The reference's
 * np.random draws are inputs (row_draws: create_tree_rows' uniform(-l_std, l_std)
 * per row; eps_draws: create_headland_countour_lines' uniform(-0.5, 0.5) per row,
 * orchard_geometry_environment.py:71).  Polygons come out in the reference's order. */
#define HTP_OGE_NPARAM 16
enum {
  HTP_OGE_P_NROWS = 0,   /* tree rows (3..32) */
  HTP_OGE_P_ROWW, HTP_OGE_P_ROWLEN, HTP_OGE_P_SLOPE,   /* create_tree_rows row_width, row_lengths, slope_angle */
  HTP_OGE_P_TREEW, HTP_OGE_P_HW,                       /* tree_width, headland_width */
  HTP_OGE_P_SX, HTP_OGE_P_SY, HTP_OGE_P_SYAW,          /* start (row-leave) pose */
  HTP_OGE_P_EX, HTP_OGE_P_EY, HTP_OGE_P_EYAW,          /* end (row-enter) pose */
  HTP_OGE_P_SIDE                                       /* 1 NEAR_SIDE, -1 FAR_SIDE */
};
#define HTP_OGE_MAXROWS 32
#define HTP_OGE_MAXPOLY 32
#define HTP_OGE_MAXV 12
enum { HTP_OGE_OK = 0, HTP_OGE_BAD_INPUT = 1, HTP_OGE_NO_ROW_BETWEEN = 2 /* reference: IndexError */,
       HTP_OGE_OVERFLOW = 3 /* more than MAXPOLY polygons or MAXV vertices */, HTP_OGE_EMPTY_SIDE = 4 };
typedef struct {
  int32_t batch, max_rows;  /* max_rows = row stride of the draw arrays */
  const double* params;     /* [batch][HTP_OGE_NPARAM] */
  const double* row_draws;  /* [batch][max_rows] */
  const double* eps_draws;  /* [batch][max_rows] */
} htp_oge_batch;
typedef struct {
  int32_t* status;          /* [batch] HTP_OGE_* */
  int32_t* n_poly;          /* [batch] */
  int32_t* n_vert;          /* [batch][MAXPOLY] */
  double* vertices;         /* [batch][MAXPOLY][MAXV][2] */
  int32_t* n_facet;         /* [batch][MAXPOLY] facets (-1: fewer than 3 distinct vertices) (nullable) */
  double* A;                /* [batch][MAXPOLY][MAXV][2] (nullable with n_facet) */
  double* b;                /* [batch][MAXPOLY][MAXV]    (nullable with n_facet) */
} htp_oge_result;
int htp_oge_obstacles_batch(htp_ctx* ctx, const htp_oge_batch* in, htp_oge_result* out);
int htp_oge_obstacles_batch_device(htp_ctx* ctx, const htp_oge_batch* in, htp_oge_result* out, void* stream);
double htp_oge_last_ms(htp_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Classic headland turns: one warm-start path per problem,
 * rows [x, y, yaw, k, dir] as the reference's planners return them (csrc/classic_core.h):
 *   HTP_CT_DUBINS      get_dubins_path_full(start, end, R, step)   safety_forward_path_plan.py:286-297
 *   HTP_CT_CIRCLEBACK  get_circle_back_path_full(start, end, R, car, side, step)   :395-454
 *   HTP_CT_FISHTAIL    get_start_end_pose_for_reeds_shepp (:300-364) + the collision-free Reeds-Shepp word
 *                      with the least backward length + Dubins lead-in/out (R/test/classic_planner.ipynb 10-11)
 * Footprints (fish-tail only): the body polygon at every pose against the blocker polygons
 * (check_path_feasibility :423-458, boundary_check=False); polygons in CSR pools as for the searches.
 *
 * Status of a turn (n_path is 0 unless HTP_CT_OK):
 *   HTP_CT_BAD_INPUT  judged before anything is planned, the turn's rows of `path` are left as they were: a
 *                     parameter that is not finite; max_steer outside (0, 1.5) or so small that the minimum
 *                     turning radius wheel_base / tan(max_steer) exceeds 1e6 m; a type other than HTP_CT_*; for
 *                     the circle-back and fish-tail types a side other than 1 / 2; wheel_base, radius or step not
 *                     positive; a body polygon of fewer than 3 or more than HTP_HA_MAX_BODY vertices; a circle-back
 *                     arc shorter than one step (the reference divides by zero there).
 *   HTP_CT_OVERFLOW   a sample or row count exceeds its capacity: Dubins samples or the fish-tail's turn-out scan
 *                     against cap_samples, the rows of an arc, a Dubins piece or the Reeds-Shepp word against
 *                     cap_path.  Counts are compared as doubles before they are converted, so a step of 1e-9 is an
 *                     overflow like any other.  The pieces that fitted before the one that did not may have been
 *                     written: rows of the turn's own [cap_path] block are unspecified, nothing outside it changes.
 *   HTP_CT_NO_WORD    no collision-free Reeds-Shepp word; HTP_CT_RS_ERROR the reference raises in reeds_shepp (nearly
 *                     coincident poses).  No row is written.
 *   HTP_CT_NO_DUBINS  no Dubins word, or a path of fewer than two distinct samples (start == end).  The Dubins type
 *                     writes no row; in the circle-back and fish-tail types the pieces before the failing Dubins
 *                     piece may have been written, as for HTP_CT_OVERFLOW.
 * Of a HTP_CT_OK turn rows [0, n_path) are written, the rows from n_path on are left as they were.  Both entries keep
 * to this: htp_classic_turn_batch hands the caller's `path`, `status` and `n_path` to the device and back. */
#define HTP_CT_NPARAM 12
enum { HTP_CT_P_TYPE = 0, HTP_CT_P_SIDE,                      /* HTP_CT_* ; map_utils NEAR_SIDE 1 / FAR_SIDE 2 */
       HTP_CT_P_SX, HTP_CT_P_SY, HTP_CT_P_SYAW, HTP_CT_P_EX, HTP_CT_P_EY, HTP_CT_P_EYAW,
       HTP_CT_P_WB, HTP_CT_P_MAXSTEER, HTP_CT_P_RADIUS, HTP_CT_P_STEP };
enum { HTP_CT_DUBINS = 0, HTP_CT_CIRCLEBACK = 1, HTP_CT_FISHTAIL = 2 };
enum { HTP_CT_OK = 0, HTP_CT_OVERFLOW = 1, HTP_CT_NO_WORD = 2 /* no collision-free word (reference: None) */,
       HTP_CT_BAD_INPUT = 3, HTP_CT_RS_ERROR = 4 /* reference raises in reeds_shepp */, HTP_CT_NO_DUBINS = 5 };
typedef struct {
  int32_t batch, npoly, nvert;
  const double* params;     /* [batch][HTP_CT_NPARAM] */
  const int32_t* desc;      /* [batch][3]: body polygon id, blockers [blk0, blk1) */
  const int32_t* poly_off;  /* [npoly+1] */
  const double* vertices;   /* [nvert][2] */
  int32_t cap_path;         /* rows per problem in `path` */
  int32_t cap_samples;      /* Dubins samples per piece (scratch sizing) */
} htp_classic_batch;
typedef struct {
  int32_t* status;          /* [batch] HTP_CT_* */
  int32_t* n_path;          /* [batch] */
  double* path;             /* [batch][cap_path][5] x, y, yaw, k, dir */
} htp_classic_result;
int htp_classic_turn_batch(htp_ctx* ctx, const htp_classic_batch* in, htp_classic_result* out);
int htp_classic_turn_batch_device(htp_ctx* ctx, const htp_classic_batch* in, htp_classic_result* out, void* stream);
double htp_classic_last_ms(htp_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Sampled exit / entry pose search of the classic turns (safety_forward_path_plan.py:457-790, the
 * sample_start_end_pose_for_dubins / _reeds_shepp / _circle_back variants; csrc/sample_core.h).
 *
 * Candidate.  A turn has base poses start = (sx, sy, syaw), end = (ex, ey, eyaw) and lists start_x[n_start],
 *   end_x[n_end].  Candidate (i, j) is start with x = start_x[i] and end with x = end_x[j]; its flattened index is
 *   i * n_end + j (the reference's loop order: start outer, end inner).  The caller builds the lists (np.arange, as
 *   the reference does); the kernel only consumes them.
 * Path of a candidate (R = params[RADIUS], the caller passes 1 / car.curvature; step = params[STEP], 0.1):
 *   HTP_SMP_DUBINS       get_dubins_path_full(start, end, R, step)
 *   HTP_SMP_REEDS_SHEPP  every word of calc_all_paths(start, end, 1 / R, step), sampled as the fish-tail samples them
 *   HTP_SMP_CIRCLE_BACK  get_circle_back_path_full(start, end, R, car, side, step); n_end == 1
 * Feasible = check_path_feasibility(car, path, boundary_check=False, aux_check=True): the body at every path row and
 *   each implement at every second row (rows 0, 2, 4, ... as get_path_poly places them) disjoint from every blocker
 *   under the closed-set separating-axis predicate of the other planners (touching collides).  No field containment.
 * Score = get_min_distance_to_boundary(car, path, with_aux=True): the minimum, over all corners of the body placed at
 *   every row and of each implement placed at every second row, of the signed distance to the field ring: Euclidean
 *   distance to the nearest ring segment, positive when the corner is inside the ring by the crossing-number rule of
 *   the searches' field test, negative otherwise.
 *   A Reeds-Shepp candidate scores the maximum over its feasible words; without a feasible word it is infeasible.
 * Winner.  Dubins / Reeds-Shepp: the feasible candidate with the largest score, ties to the lowest flattened index
 *   (the reference's strict >); none feasible: HTP_SMP_NONE_FEASIBLE (the reference returns None).  Circle-back: the
 *   first feasible candidate in index order; none feasible: the LAST candidate is reported with
 *   HTP_SMP_NONE_FEASIBLE (the reference's exhausted while loop returns the last pose it tried).
 * Deviation from the reference, stated: the reference scores exterior.coords of the shapely unary_union of the placed
 *   polygons; this scores every corner of every placed polygon.  For a CONVEX field ring the two minima are the same
 *   number (the signed distance to a convex set is concave, so its minimum over the swept region is attained at an
 *   extreme point of the region's hull, which is a placed corner on the union's exterior).  For a non-convex ring
 *   (get_map_exterior_pts with l_std > 0) they can differ: the reference adds edge-crossing points and drops interior
 *   corners.  The reference itself (shapely, pydubins) was not run against this; the numpy restatement in
 *   path_planner/safety_forward_path_plan.py is the oracle of the tests.
 * The body and the implements are 4-vertex polygons (car_model.py builds rectangles only).  Per turn, the body, the
 *   implements, the blockers and the field ring together hold at most HTP_SMP_MAX_POLY polygons and
 *   HTP_SMP_MAX_VERT vertices (they are staged in LDS); more is HTP_SMP_BAD_INPUT.
 * The winner's path is not an output: feed the safe poses to htp_classic_turn_batch. */
#define HTP_SMP_NDESC 6
#define HTP_SMP_NPOSE 8
#define HTP_SMP_MAX_POLY 48
#define HTP_SMP_MAX_VERT 256
enum { HTP_SMP_D_BODY = 0, HTP_SMP_D_AUX0, HTP_SMP_D_AUX1 /* implement polygon ids, -1: none */,
       HTP_SMP_D_BLK0, HTP_SMP_D_BLK1 /* blockers [blk0, blk1) */, HTP_SMP_D_FIELD /* field ring */ };
enum { HTP_SMP_DUBINS = 0, HTP_SMP_REEDS_SHEPP = 1, HTP_SMP_CIRCLE_BACK = 2 };
/* turn status.  OVERFLOW: n_start * n_end > cap_cand, or a candidate's path outgrew cap_samples (the winner among the
 * remaining candidates is still reported).  BAD_INPUT: non-finite base pose or car parameter, n_start or n_end out of
 * [1, cap], circle-back with n_end != 1, unknown type or side, polygons out of range or over the LDS capacity,
 * max_steer outside (0, 1.5).  htp_classic_turn_batch's further bound on max_steer (a minimum turning radius of at
 * most 1e6 m) is not applied here: a smaller max_steer is planned and ends as the planner has it (C_OVERFLOW). */
enum { HTP_SMP_OK = 0, HTP_SMP_NONE_FEASIBLE = 1, HTP_SMP_OVERFLOW = 2, HTP_SMP_BAD_INPUT = 3 };
/* candidate status.  PLANNER: no Dubins path / no Reeds-Shepp word, or the reference would raise in reeds_shepp.
 * OVERFLOW: a path longer than cap_samples.  BAD_INPUT: a non-finite x sample.  UNUSED: a table slot past
 * n_start * n_end, or any slot of a turn that ended OVERFLOW (table) or BAD_INPUT. */
enum { HTP_SMP_C_FEASIBLE = 0, HTP_SMP_C_BLOCKED = 1, HTP_SMP_C_PLANNER = 2, HTP_SMP_C_OVERFLOW = 3,
       HTP_SMP_C_BAD_INPUT = 4, HTP_SMP_C_UNUSED = 5 };
typedef struct {
  int32_t batch, npoly, nvert;
  const double* params;     /* [batch][HTP_CT_NPARAM], the HTP_CT_P_* layout with TYPE = HTP_SMP_* */
  const int32_t* desc;      /* [batch][HTP_SMP_NDESC] polygon ids */
  const int32_t* poly_off;  /* [npoly+1] */
  const double* vertices;   /* [nvert][2] */
  const double* start_x;    /* [batch][cap_s] */
  const double* end_x;      /* [batch][cap_e] */
  const int32_t* n_start;   /* [batch] */
  const int32_t* n_end;     /* [batch] */
  int32_t cap_s, cap_e;
  int32_t cap_cand;         /* candidate table slots per turn: n_start * n_end <= cap_cand */
  int32_t cap_samples;      /* path rows / Dubins samples per candidate (scratch sizing), >= 16 */
  int32_t max_groups;       /* workgroups of each candidate kernel; 0: as many as are resident at once */
} htp_classic_sample_in;
typedef struct {
  int32_t* status;          /* [batch] HTP_SMP_* */
  int32_t* winner;          /* [batch][2] i, j (-1, -1 where there is none) */
  double* poses;            /* [batch][HTP_SMP_NPOSE] safe start x, y, yaw, safe end x, y, yaw, leave_offset,
                               enter_offset (|x - base x|); NaN where there is no winner */
  double* score;            /* [batch] the winner's score (-inf where there is none) */
  int32_t* n_feasible;      /* [batch] */
  double* cand_score;       /* [batch][cap_cand] score, -inf where not feasible (nullable) */
  int32_t* cand_status;     /* [batch][cap_cand] HTP_SMP_C_* (nullable) */
} htp_classic_sample_result;
int htp_classic_sample_batch(htp_ctx* ctx, const htp_classic_sample_in* in, htp_classic_sample_result* out);
int htp_classic_sample_batch_device(htp_ctx* ctx, const htp_classic_sample_in* in, htp_classic_sample_result* out,
                                    void* stream);
double htp_classic_sample_last_ms(htp_ctx* ctx);   /* candidate kernels + winner kernel of the last launch */

/* ---------------------------------------------------------------------------
 * Maximal speed profile and timed trajectory of planner paths (no reference counterpart: the only speed a classic
 * turn gets there is get_init_ref_path's v = +-desired_v, R/obca_py/util.py:62-113; csrc/speed_core.h, DESIGN.md
 * s.3.17).  One wavefront per path, workgroups stride over the batch.
 *
 * Input per path: rows [n][5] = x, y, yaw, k, dir (dir = +-1), the layout of htp_classic_result.path, and a limits row
 *   (HTP_SPD_L_*).  A non-zero path_status entry ends the path HTP_SPD_SKIPPED, so htp_classic_result.status can be
 *   passed straight in.
 * Geometry.  ds_i = hypot(x_{i+1} - x_i, y_{i+1} - y_i); S_0 = 0, S_{i+1} = S_i + ds_i, a serial left-to-right sum (as
 *   refpath_core.h and the timeline's A_i); delta_i = atan(L k_i).  Interval i runs from node i to node i+1 in gear
 *   g_i = dir_{i+1}.  Node i is a STOP NODE when dir_{i+1} != dir_i: that row is the cusp itself (the Reeds-Shepp sampler
 *   writes the junction with the finishing segment's direction), the gap to the next row is driven in the new gear.
 * Node cap c_i = the least of
 *   VMAX        v_fwd or v_rev of each adjacent interval (by its gear);
 *   ALAT        sqrt(a_lat / |k_i|) when a_lat > 0 and k_i != 0;
 *   STEER_RATE  omega ds_j / |ddelta_j| for each adjacent interval j with ddelta_j = delta_{j+1} - delta_j != 0, when
 *               omega > 0.  The cap holds at BOTH ends of the interval, so the interval's mean speed is at most the cap
 *               and its steering rate at most omega; it is conservative by up to 2x (an interval entered from rest could
 *               leave at twice the cap).  This is what makes the curvature jumps of Dubins and Reeds-Shepp words
 *               drivable.  A zero-length interval with a steer jump caps both its nodes at exactly 0;
 *   STOP        0 at a stop node;
 *   ENDPOINT    c_0 <- min(c_0, v0), c_{n-1} <- min(c_{n-1}, v1).
 * Profile, with w = v^2: f_0 = c_0^2, f_{i+1} = min(c_{i+1}^2, f_i + 2 acc ds_i); w_{n-1} = f_{n-1},
 *   w_i = min(f_i, w_{i+1} + 2 dec ds_i); v_i = sqrt(w_i): the largest profile under the caps and the two acceleration
 *   bounds.  The library evaluates the two passes as min-plus scans, f_i = min(c_i^2, 2 acc S_i + min_{j<i}(c_j^2 -
 *   2 acc S_j)) and its mirror image with dec; the node's own c_i^2 stays outside the shifted minimum, so a stop node is
 *   exactly 0 and w_i == c_i^2 is decidable.  The scan form and the recurrence differ by rounding only.
 * Interval time dt_i:
 *   dwell  ds_i == 0: |ddelta_i| / omega (0 when omega is off or there is no jump);
 *   else   2 ds_i / (v_i + v_{i+1}) when v_i + v_{i+1} > 0: constant acceleration a_i = (w_{i+1} - w_i) / (2 ds_i);
 *   hop    both speeds 0 and ds_i > 0 (two cusps less than a step apart, or a two-row path): accelerate at acc to
 *          w_m = 2 acc dec ds_i / (acc + dec), then brake at dec: dt_i = sqrt(w_m) / acc + sqrt(w_m) / dec; a_i is
 *          reported as acc; the path gets HTP_SPD_F_HOP.
 *   t_0 = 0, t_{i+1} = t_i + dt_i, a serial sum; T = t_{n-1}.
 * Per-node outputs (nullable; rows from n_path on are left as they were): node[HTP_SPD_N_*] = S, t, signed speed g v,
 *   signed acceleration g a_i and steering rate ddelta_i / dt_i of the LEAVING interval (g = g_i; the last node takes
 *   g_{n-2}, acceleration 0 and rate 0; the rate of an interval with dt_i == 0 is 0), delta, cap c_i.
 *   active (HTP_SPD_A_*): the cap's kind when w_i == c_i^2, the first in the order STOP, VMAX, ALAT, STEER_RATE,
 *   ENDPOINT that attains the minimum; otherwise ACC when the forward bound is smaller than the backward one, else DEC.
 * Summary per path (HTP_SPD_S_*): T, S_{n-1}, forward and reverse length, number of stop nodes, total dwell time, peak
 *   speed, peak v^2 |k|, largest |delta_i|, and the time under each active kind (an interval's time is charged to its
 *   entry node).  The sums are serial, in node order.  flags: HTP_SPD_F_*.
 * Status.  HTP_SPD_BAD_INPUT: n_path < 2 or > cap_path; a non-finite double among those read (the path's rows and its
 *   limits); a dir other than +-1; L, v_fwd, v_rev, acc or dec not positive; a_lat, omega, v0 or v1 negative.  Of a
 *   HTP_SPD_SKIPPED or HTP_SPD_BAD_INPUT path only status (and count = 0, flags = 0) is written.
 * Fixed-period rows (dt > 0), the columns and the row rule of htp_obca_timeline_batch: regular rows at s = k dt (a
 *   product) while k dt < T, then exactly one final row, the last node at T (stage n-1, acceleration and steering rate
 *   of the last interval).  count = rows needed; HTP_SPD_F_TRUNCATED when count > cap_rows (the first cap_rows rows are
 *   written); T / dt >= 2^30 is HTP_SPD_F_BAD_TIME (count 0, no row).  The interval of a regular row is the largest i
 *   with t_i <= s (it has dt_i > 0).  Within it tau = s - t_i; dist = v_i tau + a_i tau^2 / 2 (a hop uses its two
 *   phases); lambda = dist / ds_i clamped to [0, 1] (a dwell: lambda = tau / dt_i, dist = 0); x, y and k are linear in
 *   lambda; theta = yaw_i + lambda wrap(yaw_{i+1} - yaw_i), wrap(d) = d - 2 pi floor((d + pi) / (2 pi));
 *   steer = atan(L k); arc = S_i + dist; v and accel are signed by g_i; steer_rate = ddelta_i / dt_i.
 * Every loop is bounded by cap_path or cap_rows. */
#define HTP_SPD_NLIM 10
#define HTP_SPD_NNODE 7
#define HTP_SPD_NKIND 7
#define HTP_SPD_NSUM 16
enum { HTP_SPD_L_WHEELBASE = 0, HTP_SPD_L_VFWD, HTP_SPD_L_VREV, HTP_SPD_L_ACC, HTP_SPD_L_DEC,
       HTP_SPD_L_ALAT /* 0: off */, HTP_SPD_L_STEER_RATE /* 0: off */, HTP_SPD_L_MAXSTEER /* flag only */,
       HTP_SPD_L_V0 /* entry speed */, HTP_SPD_L_V1 /* exit speed */ };
enum { HTP_SPD_N_S = 0, HTP_SPD_N_T, HTP_SPD_N_V, HTP_SPD_N_ACC, HTP_SPD_N_STEER, HTP_SPD_N_STEER_RATE, HTP_SPD_N_CAP };
enum { HTP_SPD_A_STOP = 0, HTP_SPD_A_VMAX, HTP_SPD_A_ALAT, HTP_SPD_A_STEER_RATE, HTP_SPD_A_ENDPOINT, HTP_SPD_A_ACC,
       HTP_SPD_A_DEC };
enum { HTP_SPD_S_T = 0, HTP_SPD_S_LENGTH, HTP_SPD_S_LEN_FWD, HTP_SPD_S_LEN_REV, HTP_SPD_S_STOPS, HTP_SPD_S_DWELL,
       HTP_SPD_S_PEAK_V, HTP_SPD_S_PEAK_LAT, HTP_SPD_S_MAX_STEER, HTP_SPD_S_TIME_KIND /* .. + HTP_SPD_NKIND */ };
enum { HTP_SPD_OK = 0, HTP_SPD_SKIPPED = 1, HTP_SPD_BAD_INPUT = 2 };
enum { HTP_SPD_F_HOP = 1, HTP_SPD_F_STEER_EXCEEDS = 2 /* some |delta_i| > max_steer */, HTP_SPD_F_TRUNCATED = 4,
       HTP_SPD_F_BAD_TIME = 8 };
typedef struct {
  int32_t batch, cap_path;
  const double* path;          /* [batch][cap_path][5] x, y, yaw, k, dir */
  const int32_t* n_path;       /* [batch] */
  const int32_t* path_status;  /* nullable [batch]: non-zero -> HTP_SPD_SKIPPED */
  const double* limits;        /* [batch][HTP_SPD_NLIM] */
  double dt;                   /* output period; 0: no fixed-period rows */
  int32_t cap_rows;            /* rows of storage per path (>= 2 when dt > 0) */
  int32_t max_groups;          /* workgroups of the launch, each with 56 cap_path bytes of device scratch kept by the
                                  context; 0: as many as are resident at once, but no more than fit 256 MiB */
} htp_speed_in;
typedef struct {
  int32_t* status;             /* [batch] HTP_SPD_* */
  int32_t* flags;              /* [batch] HTP_SPD_F_* bits */
  double* summary;             /* [batch][HTP_SPD_NSUM] */
  double* node;                /* nullable [batch][cap_path][HTP_SPD_NNODE] */
  int32_t* active;             /* nullable [batch][cap_path] HTP_SPD_A_* */
  int32_t* count;              /* [batch] fixed-period rows needed (0 when dt == 0) */
  double* rows;                /* [batch][cap_rows][HTP_TIMELINE_NCOL]; required when dt > 0 */
  int32_t* stage;              /* nullable [batch][cap_rows]: the interval of a regular row, n-1 for the final row */
} htp_speed_result;
/* API errors (-1 with a "[speed]" message, nothing launched): a null required argument, batch < 0, cap_path < 2, dt not
 * finite or < 0, dt > 0 with cap_rows < 2 or without rows, max_groups < 0.  batch == 0 returns 0. */
/* host pointers, synchronous; the caller's output arrays travel to the device and back, so what the kernel leaves
 * unwritten stays as it was */
int htp_speed_profile_batch(htp_ctx* ctx, const htp_speed_in* in, htp_speed_result* out);
/* device pointers, enqueued on `stream`, not synchronised: behind htp_classic_turn_batch_device on the same stream it
 * times that launch's path / n_path / status without a host round trip */
int htp_speed_profile_batch_device(htp_ctx* ctx, const htp_speed_in* in, htp_speed_result* out, void* stream);
/* duration (ms) of the last speed-profile kernel (hipEvents on its stream) */
double htp_speed_profile_last_ms(htp_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Clearance of pose sequences against OBCA polytopes, and the fastest admissible candidate per headland (no reference
 * counterpart: the classic planners there ignore the obstacle set the solve is held to; csrc/clear_core.h, DESIGN.md
 * s.3.18).  One wavefront per path, workgroups stride over the batch.
 *
 * Input per path p: rows poses[p][cap_poses][stride] with a launch-uniform stride >= 3 and the columns col_x, col_y,
 *   col_yaw (distinct, < stride): planner paths [x, y, yaw, k, dir] are stride 5, columns (0, 1, 2); fixed-period rows
 *   of either kind of turn are stride HTP_TIMELINE_NCOL, columns (1, 2, 4).  n = min(n_poses[p], cap_poses) poses are
 *   used and HTP_CLR_F_TRUNCATED is set when n_poses[p] > cap_poses, so htp_speed_result.count can be passed straight
 *   in.  A non-zero pose_status entry ends the path HTP_CLR_SKIPPED, so htp_classic_result.status or the speed status
 *   goes straight in.  scene[p] (nullable: scene[p] = p, which requires n_scenes == batch) names the obstacle / body
 *   set of the path, so several candidate turns of one headland share one set.
 * Scenes: n_scenes sets of M <= 16 obstacles and K <= 4 bodies as halfspaces in the layout of htp_obca_batch: obs_A,
 *   obs_b, body_G, body_g indexed by scene (obs_edges / body_edges are host arrays, launch-uniform, 3..8 each), turned
 *   into edges by the audit's rule (rows of any order, possibly redundant); margin[n_scenes] nullable, finite, may be
 *   negative.
 * Poses measured: the n given poses and, with substeps S > 1, S-1 poses inside every gap i -> i+1: for q = 1..S-1,
 *   lam = (double)q / S, x = x_i + lam (x_{i+1} - x_i), y likewise, yaw = yaw_i + lam wrap(yaw_{i+1} - yaw_i) with the
 *   speed block's wrap(d) = d - 2 pi floor((d + pi) / (2 pi)).  The yaw column is the vehicle's heading, on reverse
 *   segments too.  Each pose places every body (the audit's signed distance of two convex polygons: the sign is exact,
 *   the magnitude is the distance when they are disjoint and minus the penetration depth otherwise).
 * Outputs.  status HTP_CLR_*: BAD_INPUT is n < 1, a non-finite double among those read (the three columns of the n
 *   poses, the scene's rows, its margin) or a scene index outside 0..n_scenes-1; BAD_POLYTOPE is an empty or unbounded
 *   obstacle or body.  flags HTP_CLR_F_*: COLLISION clearance < 0; MARGIN margin given and clearance < margin -
 *   margin_tol; TRUNCATED.  metrics[HTP_CLR_*]: CLEARANCE the least signed distance over all poses and (obstacle, body)
 *   pairs, CLEARANCE_NODE the same over the given poses only, MAX_GAP the largest hypot between consecutive given
 *   poses and MAX_TURN the largest |wrap(yaw_{i+1} - yaw_i)| (both 0 for n == 1: they tell whether S was enough).
 *   worst[4]: pose, substep, obstacle and body of CLEARANCE, ties to the lowest tuple.  pose_clearance (nullable)
 *   [cap_poses]: the least over the pairs for pose i and the substeps of the gap it opens.  Of a path that is not
 *   HTP_CLR_OK only status and flags = 0 are written; entries from n on are never written.
 * Every reduction is a minimum or a maximum: the result does not depend on lane order, chunking or workgroup count. */
#define HTP_CLR_NMETRIC 4
#define HTP_CLR_MAX_SUBSTEPS 16
enum { HTP_CLR_CLEARANCE = 0, HTP_CLR_CLEARANCE_NODE, HTP_CLR_MAX_GAP, HTP_CLR_MAX_TURN };
enum { HTP_CLR_OK = 0, HTP_CLR_SKIPPED = 1, HTP_CLR_BAD_INPUT = 2, HTP_CLR_BAD_POLYTOPE = 3 };
enum { HTP_CLR_F_COLLISION = 1, HTP_CLR_F_MARGIN = 2, HTP_CLR_F_TRUNCATED = 4 };
typedef struct {
  int32_t batch, cap_poses, stride, col_x, col_y, col_yaw;
  const double* poses;         /* [batch][cap_poses][stride] */
  const int32_t* n_poses;      /* [batch] */
  const int32_t* pose_status;  /* nullable [batch]: non-zero -> HTP_CLR_SKIPPED */
  const int32_t* scene;        /* nullable [batch]: the path's scene; null: scene[p] = p */
  int32_t n_scenes, M, K;
  const int32_t* obs_edges;    /* [M] host array, 3..8 each */
  const int32_t* body_edges;   /* [K] host array, 3..8 each */
  const double* obs_A;         /* [n_scenes][sum obs_edges][2] */
  const double* obs_b;         /* [n_scenes][sum obs_edges] */
  const double* body_G;        /* [n_scenes][sum body_edges][2] */
  const double* body_g;        /* [n_scenes][sum body_edges] */
  const double* margin;        /* nullable [n_scenes] */
  int32_t substeps;            /* S, 1..HTP_CLR_MAX_SUBSTEPS */
  double margin_tol;           /* >= 0 */
  int32_t max_groups;          /* workgroups of the launch; 0: as many as are resident at once */
} htp_clear_in;
typedef struct {
  int32_t* status;             /* [batch] HTP_CLR_* */
  int32_t* flags;              /* [batch] HTP_CLR_F_* bits */
  double* metrics;             /* [batch][HTP_CLR_NMETRIC] */
  int32_t* worst;              /* [batch][4] pose, substep, obstacle, body */
  double* pose_clearance;      /* nullable [batch][cap_poses] */
} htp_clear_result;
/* API errors (-1 with a "[clearance]" message, nothing launched): a null required argument, batch < 0, cap_poses < 1,
 * a bad stride or column, M, K or an edge count out of range, n_scenes < 1, a null scene with n_scenes != batch,
 * substeps out of range, a negative (or non-finite) tolerance, max_groups < 0, cap_poses * substeps * M * K >= 2^31
 * (the index of the worst pose is an int32).  batch == 0 returns 0. */
/* host pointers, synchronous; the caller's output arrays travel to the device and back, so what the kernel leaves
 * unwritten stays as it was */
int htp_pose_clearance_batch(htp_ctx* ctx, const htp_clear_in* in, htp_clear_result* out);
/* device pointers (obs_edges / body_edges stay host arrays), enqueued on `stream`, not synchronised */
int htp_pose_clearance_batch_device(htp_ctx* ctx, const htp_clear_in* in, htp_clear_result* out, void* stream);
/* duration (ms) of the last clearance kernel (hipEvents on its stream) */
double htp_pose_clearance_last_ms(htp_ctx* ctx);

/* The fastest admissible candidate per problem.  batch B problems with C candidates each (1..8); candidate c of
 * problem b sits at index c B + b in every input array (the layout of C B paths planned, timed and measured in one
 * launch each).  Verdict per candidate (verdict[B][C], HTP_SEL_* bits; 0: admissible):
 *   NOT_PLANNED  speed status HTP_SPD_SKIPPED;
 *   BAD          speed status neither HTP_SPD_OK nor HTP_SPD_SKIPPED (HTP_SPD_BAD_INPUT), or clearance status not
 *                HTP_CLR_OK;
 *   SPEED_FLAG   the speed flags hit reject_speed_flags; CLEAR_FLAG the clearance flags hit reject_clear_flags;
 *   TOO_LONG     t_max > 0 and T > t_max; NONFINITE T is not finite, where T = spd_summary[HTP_SPD_S_T] is read only
 *                of a candidate whose speed status is HTP_SPD_OK (the speed profile writes no summary otherwise).
 * winner[B]: the admissible candidate of least T, an equal T goes to the lowest c; -1 without one.  score[B]: its T,
 * or NaN.  clearance[B] (nullable; needs clr_metrics): its HTP_CLR_CLEARANCE, or NaN.  With rows, the winner's first
 * min(count, cap_rows) rows are copied to out_rows[B][cap_rows][HTP_TIMELINE_NCOL] and out_count[B] is its count (0
 * without a winner); rows beyond that are left as they were.  One wavefront per problem; no reduction. */
#define HTP_SEL_MAX_CAND 8
enum { HTP_SEL_NOT_PLANNED = 1, HTP_SEL_BAD = 2, HTP_SEL_SPEED_FLAG = 4, HTP_SEL_CLEAR_FLAG = 8, HTP_SEL_TOO_LONG = 16,
       HTP_SEL_NONFINITE = 32 };
typedef struct {
  int32_t batch, C;
  const int32_t* spd_status;   /* [C][batch] */
  const int32_t* spd_flags;    /* [C][batch] */
  const double* spd_summary;   /* [C][batch][HTP_SPD_NSUM] */
  const double* rows;          /* nullable [C][batch][cap_rows][HTP_TIMELINE_NCOL] */
  const int32_t* count;        /* [C][batch]; required with rows */
  int32_t cap_rows;            /* >= 1 with rows */
  const int32_t* clr_status;   /* [C][batch] */
  const int32_t* clr_flags;    /* [C][batch] */
  const double* clr_metrics;   /* nullable [C][batch][HTP_CLR_NMETRIC] */
  int32_t reject_speed_flags, reject_clear_flags;
  double t_max;                /* 0: off */
} htp_select_in;
typedef struct {
  int32_t* verdict;            /* [batch][C] HTP_SEL_* bits */
  int32_t* winner;             /* [batch] */
  double* score;               /* [batch] */
  double* clearance;           /* nullable [batch] */
  double* out_rows;            /* [batch][cap_rows][HTP_TIMELINE_NCOL]; required with rows */
  int32_t* out_count;          /* [batch]; required with rows */
} htp_select_result;
/* API errors (-1 with a "[select]" message, nothing launched): a null required argument, batch < 0, C outside 1..8,
 * rows without count, out_rows, out_count or cap_rows >= 1, clearance without clr_metrics, t_max negative or NaN. */
int htp_turn_select_batch(htp_ctx* ctx, const htp_select_in* in, htp_select_result* out);
int htp_turn_select_batch_device(htp_ctx* ctx, const htp_select_in* in, htp_select_result* out, void* stream);
double htp_turn_select_last_ms(htp_ctx* ctx);

/* ---------------------------------------------------------------------------
 * Orchard workload chain on the device (synth.make_orchard_instance's steps after the scene draws): for each
 * problem, the classic turn (htp_classic_turn_batch) -> get_init_ref_path at spacing ds / 2 = L / (2N - 2)
 * (ds = L / (N - 1), the resampled spacing), desired_v = min(ds / dT, 0.9) (R/obca_py/util.py:62-113) -> the init guess resampled to N rows and the
 * headland width the warm start needs -> the OGE_OBCA obstacle producer (htp_oge_obstacles_batch) -> quads,
 * the M nearest, halfspaces.  Writes the htp_obca_batch arrays traj / obs_A / obs_b (4 edges per obstacle)
 * in HBM, enqueued on `stream`; intermediates live in the context.  `scenes` and `turns` hold device
 * pointers; scenes.params[b][HTP_OGE_P_HW] is overwritten with the chain's headland width. */
typedef struct {
  int32_t batch, N, M;
  htp_oge_batch scenes;            /* device */
  htp_classic_batch turns;         /* device pools */
  const double* margin;            /* [batch] device: boundary margin behind the warm start */
  int32_t n_vpoly;                 /* vehicle footprint polygons (car frame): body, then the implement (<= 2) */
  int32_t vpoly_nv[2];
  double vpoly[2][8][2];
  double dT, wheel_base;
  int32_t cap_rows;                /* init-guess rows per problem */
  double* traj;                    /* [batch][N][5] device out */
  double* obs_A;                   /* [batch][4 M][2] device out */
  double* obs_b;                   /* [batch][4 M] device out */
  int32_t* status;                 /* [batch] device out: 0, or 16 * stage + that stage's status
                                      (stage 1 classic, 2 init guess, 3 obstacle producer, 4 quads) */
} htp_chain_batch;
int htp_orchard_chain_device(htp_ctx* ctx, const htp_chain_batch* in, void* stream);
double htp_chain_last_ms(htp_ctx* ctx);


/* ---------------------------------------------------------------------------
 * The notebook planner chain on the device (R/path_planner/headland_path_planning.py:124-255, the planner of
 * R/test/obca.ipynb cells 9-15): for each problem, the Y-type parking search (htp_ypark_search_batch_device)
 * fixes the intermediate pose; the heuristic lowering (csrc/ychain_core.h: get_topology_waypoints, the
 * ReferenceLineHeuristic guide path, segment lanes and search lengths) writes the hybrid A* inputs of that
 * problem into reserved slots of the search's pools; the hybrid A* search (htp_hastar_search_batch_device) runs
 * from the start to the intermediate pose; its path and the parking manoeuvre are joined and turned into the
 * init guess (get_init_ref_path, refpath_core.h) and resampled to N rows (the OBCA solve's traj input).
 * Everything stays in HBM; four launches on `stream`.  Reserved hybrid A* slots of problem b: polygon ids
 * [lane_poly0 + b * HTP_YC_POLY_STRIDE, + HTP_YC_POLY_STRIDE) (the last one spans the unused vertices),
 * vertices [lane_vert0 + b * HTP_YC_VERT_STRIDE, ...), guide rows [guide0 + b * guide_stride, ...); the host
 * sets hastar.poly_off at every problem's first slot id (and at lane_poly0 + batch * HTP_YC_POLY_STRIDE), the
 * device writes the rest, hastar.params[b] GX..GYAW and hastar.desc[b] LANE0..GUIDE1. */
#define HTP_YC_MAXWP 10
#define HTP_YC_POLY_STRIDE HTP_YC_MAXWP
#define HTP_YC_VERT_STRIDE ((HTP_YC_MAXWP - 1) * 80)
typedef struct {
  int32_t batch, N;
  htp_ypark_batch ypark;            /* device arrays */
  htp_ypark_result ypark_out;       /* device arrays (path: [batch][ypark.cap_path][5]) */
  htp_hastar_batch hastar;          /* device pools; the lane / guide slots and GX..GYAW, LANE0..GUIDE1 are written */
  htp_hastar_result hastar_out;     /* device arrays (paths: [batch][hastar.cap_path]) */
  const double* rows;               /* [batch][max_rows][4]: near x, near y, far x, far y of every tree row */
  const int32_t* nrows;             /* [batch] */
  const double* eps;                /* [batch][max_rows]: check_side_of_a_point's uniform(-0.5, 0.5) draws */
  const double* start;              /* [batch][3] the search start pose */
  int32_t max_rows;
  double drive_row_offset;          /* headland_planner_y_type_park's drive_row_offset */
  int32_t lane_poly0, lane_vert0, guide0, guide_stride;
  const double* rp_params;          /* [batch][3] WHEEL_BASE, desired_v, ds (get_init_ref_path) */
  int32_t cap_rows;                 /* init-guess rows per problem */
  double* ref;                      /* [batch][cap_rows][5] init guess out (get_init_ref_path rows) */
  int32_t* n_ref;                   /* [batch] */
  double* traj;                     /* [batch][N][5] the init guess resampled to N rows (OBCA traj) */
  int32_t* status;                  /* [batch]: 0, or 16 * stage + that stage's status (1 Y-park, 2 lowering,
                                       3 hybrid A*, 4 init guess) */
} htp_ychain_batch;
int htp_ypark_hastar_chain_device(htp_ctx* ctx, const htp_ychain_batch* in, void* stream);
/* Per-stage kernel times (ms) of the last chain: Y-park, lowering, hybrid A*, init guess + resample. */
int htp_ychain_last_ms(htp_ctx* ctx, double* ms4);

/* ---- deterministic double-double libm of the planner cores (csrc/htp_libm.h) ----------------------------------------
 * Replaces nothing in the reference: the reference's planners call CPython's math module / numpy (glibc, or
 * numpy's SIMD kernels), whose last bits differ between platforms.  Every device planner kernel and every host
 * build of the same cores evaluates sin, cos, tan, atan, atan2, asin, acos, hypot and pow with this one
 * double-double implementation (< 2^-100 relative before one final rounding, no Ziv fallback; the same
 * operations on both sides, so the same doubles), so integer outputs that hang on the last bit (a spline piece's sample
 * count, R/path_planner/utils/cubic_spline.py:102) are identical on the GPU and on the host.
 * fn: 0 sin, 1 cos, 2 tan, 3 atan, 4 atan2(x[i], y[i]), 5 asin, 6 acos, 7 hypot(x[i], y[i]), 8 pow(x[i], y[i]), 9 log; the solver's
 * fast deterministic functions (htp_fastm.h, <= 2 ulp): 10 log, 11 sin, 12 cos, 13 tan.
 * x, y, out: device arrays of n doubles (y only for the two-argument functions). */
int htp_libm_batch_device(htp_ctx* ctx, int32_t fn, const double* x, const double* y, double* out, int64_t n,
                          void* stream);

/* The fp64 matrix-core op of the solver's Riccati recursion (v_mfma_f64_16x16x4f64) on n caller tiles:
 * D[t] = A[t] (16x4, row-major) * B[t] (4x16, row-major) + C[t] (16x16, row-major), device arrays.  A
 * diagnostic surface with no reference counterpart: it pins the host model of the op's rounding that the
 * bit-exact host emulation of the device solver uses (tests/test_gpu_mfma_model.py). */
int htp_mfma_f64_probe(htp_ctx* ctx, const double* A, const double* B, const double* C, double* D, int64_t n,
                       void* stream);

/* The solver's small dense factorizations (csrc/obca_core.h) on `count` caller blocks, one block per lane of
 * 64-lane workgroups, the LDS laid out as the solver lays out its wave's (csrc/bk_probe.h).  A diagnostic
 * surface with no reference counterpart (tests/test_gpu_bk.py).  variant: 0 the unpivoted LDL^T of the local
 * blocks (n 10, 4, 8); 1 bk_factor_packed / bk_solve_packed on a private array (n 4, 8, 10, 18); 2 the same on the
 * lane-contiguous LDS slice (n 10); 3 bk_factor_simd / bk_solve_simd; 4 bk_factor_batch / bk_solve_batch, and
 * bk_solve_batch_multi into x2 when nrhs == 4 (3, 4: n 10 with lane_stride 64 or 1, n 18 with lane_stride 1);
 * 5 bk_factor_batch_p / bk_solve_batch_l (n 10, lane_stride 64 or 1); 6 chol3 / chol3_solve (n = nv = 1, 2, 3);
 * 7 chol5 / chol5_fwd (x2) / chol5_bwd (n 5).  lane_stride 64: the blocks interleaved in LDS; 1: private arrays.
 * Device arrays: K0 [count][n (n + 1) / 2] packed lower (6: [count][9], 3 x 3 stride 3; 7: [count][25]);
 * rhs [count][nrhs][n], nrhs <= 4; K the factor, in K0's layout (7: [count][15] packed); ip [count][n] pivots in
 * LAPACK dsytf2's convention, 0-based (k, or -(kp + 1) twice for a 2 x 2 pivot); flags [count][4] = negative
 * pivots, zero pivot, `piv`, Cholesky success (-1 where the form has none); x, x2 [count][nrhs][n].  Rows of
 * blocks past `count` and outputs a form does not produce are left untouched. */
int htp_bk_probe(htp_ctx* ctx, int32_t variant, int32_t n, int32_t lane_stride, int64_t count, int32_t nrhs,
                 const double* K0, const double* rhs, double* K, int32_t* ip, int32_t* flags, double* x, double* x2,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HTP_H_ */
