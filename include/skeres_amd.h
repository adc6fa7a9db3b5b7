/*
 * skeres_amd.h — C ABI of libskeres_amd.so, the MI355X (gfx950) replacement for
 * the SWIG/JNI module `ceres` + native libceres that fgcallari/skeres binds.
 *
 * Every entry point states the reference interface it replaces.  Paths are
 * relative to the reference repository:
 *   ceres.i
 *   CORE = core/src/main/scala/org/somelightprojections/skeres
 *   EX   = examples/src/main/scala/org/somelightprojections/skeres/examples
 *
 * Conventions:
 *   - plain pointers and sizes only; no C++ types, no exceptions cross the ABI;
 *   - functions returning `int` return an sk_status (0 == SK_OK) unless the
 *     comment says "boolean"; sk_last_error() holds the message of the last
 *     failure on the calling thread;
 *   - parameter memory is CALLER-OWNED host memory, identified by address, and
 *     is updated in place when sk_solve returns (README.md:51-55);
 *   - cost / loss objects are caller-owned; a Problem never frees them
 *     (CORE/Problem.scala:7-13);
 *   - one caller thread per problem / solver handle; sk_solve blocks;
 *   - there is NO CPU fallback: every compute entry point needs a gfx950 device
 *     and fails with SK_ERR_NO_DEVICE without one.
 */
#ifndef SKERES_AMD_H
#define SKERES_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum sk_status {
  SK_OK = 0,
  SK_ERR_INVALID_ARGUMENT = 1, /* JVM side: require(...) -> IllegalArgumentException */
  SK_ERR_NO_DEVICE = 2,
  SK_ERR_HIP = 3,
  SK_ERR_UNSUPPORTED = 4,
  SK_ERR_EVALUATION_FAILED = 5,
  SK_ERR_COMM = 6
} sk_status;

/* ceres::LinearSolverType (ceres/types.h, %include'd at ceres.i:137);
 * used at EX/SimpleBundleAdjuster.scala:148, EX/CurveFitting.scala:121 */
typedef enum sk_linear_solver_type {
  SK_DENSE_NORMAL_CHOLESKY = 0,
  SK_DENSE_QR = 1,
  SK_SPARSE_NORMAL_CHOLESKY = 2, /* not implemented: SK_ERR_UNSUPPORTED */
  SK_DENSE_SCHUR = 3,
  SK_SPARSE_SCHUR = 4,    /* not implemented */
  SK_ITERATIVE_SCHUR = 5, /* not implemented */
  SK_CGNR = 6             /* conjugate gradients on the normal equations over the block-sparse Jacobian */
} sk_linear_solver_type;

/* ceres::PreconditionerType, the two that CGNR takes */
typedef enum sk_preconditioner_type { SK_IDENTITY = 0, SK_JACOBI = 1 } sk_preconditioner_type;

/* ceres::MinimizerType; EX/Powell.scala:78 */
typedef enum sk_minimizer_type { SK_LINE_SEARCH = 0, SK_TRUST_REGION = 1 } sk_minimizer_type;

/* ceres::TrustRegionStrategyType and ceres::DoglegType (ceres/types.h, %include'd at ceres.i:137) */
typedef enum sk_trust_region_strategy_type { SK_LEVENBERG_MARQUARDT = 0, SK_DOGLEG = 1 } sk_trust_region_strategy_type;
typedef enum sk_dogleg_type {
  SK_TRADITIONAL_DOGLEG = 0,
  SK_SUBSPACE_DOGLEG = 1 /* not implemented: SK_ERR_UNSUPPORTED when the solver is created */
} sk_dogleg_type;

/* ceres::TerminationType, reported through Solver::Summary */
typedef enum sk_termination_type {
  SK_CONVERGENCE = 0,
  SK_NO_CONVERGENCE = 1,
  SK_FAILURE = 2,
  SK_USER_SUCCESS = 3,
  SK_USER_FAILURE = 4
} sk_termination_type;

/* ceres::Ownership; CORE/Problem.scala:10-13 forces DO_NOT_TAKE_OWNERSHIP */
typedef enum sk_ownership { SK_DO_NOT_TAKE_OWNERSHIP = 0, SK_TAKE_OWNERSHIP = 1 } sk_ownership;

/* Device functor registry.  In the reference the functor
 * body is a JVM closure reached through the SWIG director upcall
 * (ceres.i:48); a GPU cannot call it, so each functor on the hot path is a
 * device template instantiated for double and Jet<N>, addressed by id, with
 * its captured doubles passed as `consts`. */
typedef enum sk_functor_id {
  SK_FUNCTOR_HOST_CALLBACK = 0,           /* sk_cost_function_new_callback */
  SK_FUNCTOR_SNAVELY_REPROJECTION = 1,    /* EX/SimpleBundleAdjuster.scala:79-119; consts (observedX, observedY) */
  SK_FUNCTOR_EXPONENTIAL_RESIDUAL = 2,    /* EX/CurveFitting.scala:92-98; consts (x, y) */
  SK_FUNCTOR_POWELL_F1 = 3,               /* EX/Powell.scala:14-21 */
  SK_FUNCTOR_POWELL_F2 = 4,               /* EX/Powell.scala:24-31 */
  SK_FUNCTOR_POWELL_F3 = 5,               /* EX/Powell.scala:34-42 */
  SK_FUNCTOR_POWELL_F4 = 6,               /* EX/Powell.scala:45-53 */
  SK_FUNCTOR_BINARY_SCALAR_COST = 7,      /* core/src/test/.../AutodiffCostFuntionSpec.scala:14-26; consts (a) */
  SK_FUNCTOR_BINARY_VECTOR3_COST = 8,     /* AutodiffCostFuntionSpec.scala:55-69; consts (a) */
  SK_FUNCTOR_TEN_PARAMETER_COST = 9,      /* AutodiffCostFuntionSpec.scala:111-119 */
  /* BASELINE.json config 5 (synthetic dense problem; no reference counterpart): one residual
   * r = tanh(a . x) - y over ONE parameter block of any size n, the row a regenerated on the
   * device from a counter-based generator; consts (seed, row index, y).  Added with
   * sk_problem_add_dense_rows. */
  SK_FUNCTOR_SYNTH_TANH_ROW = 10,
  SK_FUNCTOR_HELLO_WORLD = 11,            /* EX/HelloWorld.scala:11-14: r = 10 - x */
  SK_FUNCTOR_QUATERNION_ROTATION = 12,    /* r = R(q) p - t, q = (w, x, y, z) normalised; consts (p[3], t[3]); no reference
                                           * counterpart: a 4-parameter block for the local parameterizations */
  SK_FUNCTOR_TAPE = 13                    /* a recorded functor body: sk_cost_function_new_tape */
} sk_functor_id;

/* A recorded functor body ("tape").  CORE/CostFunctor.scala:40-51 lets the user write ANY residual as
 *   def apply[T: Field: Trig: NRoot: Order: ClassTag](x: Array[T]*): Array[T]
 * and the reference calls it back per residual block on the JVM (ceres.i:48).  The functors of the reference's own
 * examples have device bodies above; every other functor gets to the device by being run ONCE with a recording T
 * (the Scala side: a T whose Field / Trig / NRoot instances append an instruction and return a fresh register;
 * skeres_amd/tape.py is that recording T in Python) — the list of instructions is the tape, evaluated on the GPU per
 * residual block by forward-mode autodiff exactly as CORE/AutodiffCostFunction.scala:96-130 seeds and reads its Jets.
 * An instruction is five 32-bit integers: opcode, destination register, operands a, b, c.
 * An operand is kind << 28 | index: */
typedef enum sk_tape_operand_kind {
  SK_TAPE_REGISTER = 0,   /* a register written by an earlier instruction */
  SK_TAPE_PARAMETER = 1,  /* x(i)(j), numbered through the blocks: index = N(0) + ... + N(i-1) + j */
  SK_TAPE_CAPTURED = 2,   /* the index-th double the closure captures (observedX, observedY, ...), per residual block */
  SK_TAPE_CONSTANT = 3    /* the index-th literal of the body (tape_constants) */
} sk_tape_operand_kind;
typedef enum sk_tape_opcode {
  SK_TAPE_MOV = 0, SK_TAPE_ADD, SK_TAPE_SUB, SK_TAPE_MUL, SK_TAPE_DIV, SK_TAPE_NEG, SK_TAPE_SQRT, SK_TAPE_EXP, SK_TAPE_LOG,
  SK_TAPE_SIN, SK_TAPE_COS, SK_TAPE_TAN, SK_TAPE_ASIN, SK_TAPE_ACOS, SK_TAPE_ATAN, SK_TAPE_ATAN2 /* atan2(a, b) */, SK_TAPE_ABS,
  SK_TAPE_LT,     /* 1 if real(a) <  real(b) else 0: spire's Order[Jet] compares real parts (CORE/Rotation.scala:458) */
  SK_TAPE_LE,     /* 1 if real(a) <= real(b) else 0 */
  SK_TAPE_SELECT  /* real(a) != 0 ? b : c — a data-dependent `if` of the body, BOTH of whose arms are on the tape */
} sk_tape_opcode;

typedef struct sk_ptrvec sk_ptrvec;
typedef struct sk_loss_function sk_loss_function;
typedef struct sk_cost_function sk_cost_function;
typedef struct sk_local_parameterization sk_local_parameterization;
typedef struct sk_problem sk_problem;
typedef struct sk_options sk_options;
typedef struct sk_summary sk_summary;
typedef struct sk_solver sk_solver;
typedef int sk_residual_block_id; /* CORE/package.scala:13 ResidualBlockId */

/* ---- library ------------------------------------------------------------ */
const char* sk_version(void);
const char* sk_last_error(void);
/* ceres.i:131-135 initGoogleLogging(name): kept for call-site compatibility
 * (EX/SimpleBundleAdjuster.scala:128); records the program name only. */
void sk_init_logging(const char* name);
/* Number of visible gfx950 devices (0 when none); does not fail. */
int sk_device_count(void);

/* ---- DoubleArray: ceres.i:95-96 %array_class(double, DoubleArray) -------- */
double* sk_array_new(int n);                         /* new DoubleArray(n) */
void sk_array_free(double* a);                       /* DoubleArray.delete() */
double sk_array_getitem(const double* a, int i);     /* getitem; CORE/RichDoubleArray.scala:20 */
void sk_array_setitem(double* a, int i, double v);   /* setitem; CORE/RichDoubleArray.scala:27 */
/* DoubleArraySlice.get(buffer, start) == &buffer[start]; ceres.i:99-107,
 * CORE/RichDoubleArray.scala:52.  Non-owning interior pointer. */
double* sk_array_slice(double* buffer, int start);
/* Bulk forms of CORE/RichDoubleArray.scala:36-39 (copyFrom) and :65-69
 * (toArray), so a JVM caller crosses JNI once instead of once per element. */
void sk_array_copy_in(double* dst, const double* src, int n);
void sk_array_copy_out(const double* src, double* dst, int n);

/* ---- DoubleMatrix: ceres.i:113-125 -------------------------------------- */
int sk_matrix_is_null(double* const* matrix);        /* boolean */
double* sk_matrix_row(double* const* matrix, int i);

/* ---- StdVectorDoublePointer: ceres.i:82 (std::vector<double*>) ----------- */
sk_ptrvec* sk_ptrvec_new(void);
void sk_ptrvec_free(sk_ptrvec* v);
void sk_ptrvec_add(sk_ptrvec* v, double* p);         /* CORE/Problem.scala:24-25 */
int sk_ptrvec_size(const sk_ptrvec* v);
double* sk_ptrvec_get(const sk_ptrvec* v, int i);
void sk_ptrvec_set(sk_ptrvec* v, int i, double* p);  /* CORE/RichDoubleMatrix.scala:74-75 */
double** sk_ptrvec_to_pointer_pointer(sk_ptrvec* v); /* DoubleMatrix.toPointerPointer; NULL when empty */

/* ---- Rotation (CORE/Rotation.scala:63-522) ----------------------------------------------
 * The conversion / rotation functions device functors call (csrc/rotation.hpp), evaluated ON THE DEVICE for
 * `n` inputs at once.  jet_dim 0: `in` is [n][in_len] doubles, `out` [n][out_len].  jet_dim K in 1..4: every
 * value is a Jet, stored as (real, K infinitesimal parts): in [n][in_len][1+K], out [n][out_len][1+K] — what
 * the functions compute under automatic differentiation (RotationSpec.scala:459-562).  Quaternions are
 * (w, x, y, z); 3x3 matrices are 9 values, column-major unless row_major != 0 (the reference's
 * ColumnMajorMatrixAdapter3x3 / RowMajorMatrixAdapter3x3); Euler angles are (pitch, roll, yaw) in degrees.
 * Input layout of the two-argument functions: first argument, then second (q then pt; z then w; x then y). */
typedef enum {
  SK_ROT_ANGLE_AXIS_TO_QUATERNION = 0,         /* :72   3 -> 4 */
  SK_ROT_QUATERNION_TO_ANGLE_AXIS = 1,         /* :104  4 -> 3 */
  SK_ROT_ROTATION_MATRIX_TO_QUATERNION = 2,    /* :162  9 -> 4 */
  SK_ROT_ROTATION_MATRIX_TO_ANGLE_AXIS = 3,    /* :203  9 -> 3 */
  SK_ROT_ANGLE_AXIS_TO_ROTATION_MATRIX = 4,    /* :211  3 -> 9 */
  SK_ROT_EULER_ANGLES_TO_ROTATION_MATRIX = 5,  /* :269  3 -> 9 */
  SK_ROT_QUATERNION_TO_SCALED_ROTATION = 6,    /* :326  4 -> 9 */
  SK_ROT_QUATERNION_TO_ROTATION = 7,           /* :364  4 -> 9; the zero quaternion is SK_ERR_EVALUATION_FAILED (`require`) */
  SK_ROT_UNIT_QUATERNION_ROTATE_POINT = 8,     /* :393  4+3 -> 3 */
  SK_ROT_QUATERNION_ROTATE_POINT = 9,          /* :422  4+3 -> 3 */
  SK_ROT_QUATERNION_PRODUCT = 10,              /* :435  4+4 -> 4 */
  SK_ROT_CROSS_PRODUCT = 11,                   /* :441  3+3 -> 3 (the mathematical product; the reference's first component is a typo) */
  SK_ROT_DOT_PRODUCT = 12,                     /* :445  3+3 -> 1 */
  SK_ROT_ANGLE_AXIS_ROTATE_POINT = 13          /* :449  3+3 -> 3 */
} sk_rotation_op;
int sk_rotation_apply(int op, int row_major, int jet_dim, const double* in, int n, double* out);

/* ---- LossFunction: PredefinedLossFunctions, ceres.i:168-184 -------------- */
sk_loss_function* sk_loss_trivial(void);             /* trivialLoss(): rho(s) = s; caller frees (%newobject, ceres.i:160) */
sk_loss_function* sk_loss_huber(double a);           /* huberLoss(a), ceres.i:171 */
sk_loss_function* sk_loss_soft_l_one(double a);      /* softLOneLoss(a), ceres.i:172 */
sk_loss_function* sk_loss_cauchy(double a);          /* cauchyLoss(a), ceres.i:173 */
sk_loss_function* sk_loss_tukey(double a);           /* tukeyLoss(a), ceres.i:174 */
sk_loss_function* sk_loss_tolerant(double a, double b); /* tolerantLoss(a, b), ceres.i:175 */
/* composedLoss(f, g): rho(s) = f(g(s)); scaledLoss(rho, a): a * rho(s), rho may be NULL (= a * s), ceres.i:176-182.
 * The reference builds both with DO_NOT_TAKE_OWNERSHIP; here the arguments are COPIED, so they may be freed
 * at once.  Nesting deeper than 4 is SK_ERR_UNSUPPORTED (NULL + sk_last_error). */
sk_loss_function* sk_loss_composed(const sk_loss_function* f, const sk_loss_function* g);
sk_loss_function* sk_loss_scaled(const sk_loss_function* rho, double a);
/* ceres::LossFunction::Evaluate(sq_norm, rho[3]) for n squared norms: rho + 3*i receives rho(s_i), rho'(s_i), rho''(s_i).
 * Evaluated ON THE DEVICE by the code the solvers run (known-answer tests). */
int sk_loss_evaluate(const sk_loss_function* loss, const double* sq_norm, int n, double* rho);
void sk_loss_free(sk_loss_function* loss);

/* ---- LocalParameterization: PredefinedLocalParameterizations, ceres.i:186-210 -------------
 * identity(size), subset(size, constant_parameters), quaternion(), homogeneousVector(size) — the Ceres 1.x classes
 * the reference creates through SWIG for ceres::Problem::AddParameterBlock / SetParameterization, which its Problem
 * inherits (CORE/Problem.scala:16).  Global size at most 16.  Creation returns NULL (sk_last_error) on the argument
 * errors Ceres checks: subset indices out of range or duplicated, a homogeneous vector of size < 2.  The objects
 * are copied into a problem when set; free them any time after.
 * Plus(x, delta) and ComputeJacobian(x) (global x local, row-major) are evaluated ON THE DEVICE — the code the solver
 * runs — for n points at once: x [n][global], delta [n][local] (one unused value per point when local is 0). */
sk_local_parameterization* sk_local_parameterization_identity(int size);
sk_local_parameterization* sk_local_parameterization_subset(int size, const int* constant_parameters, int num_constant);
sk_local_parameterization* sk_local_parameterization_quaternion(void);          /* (w, x, y, z) */
sk_local_parameterization* sk_local_parameterization_homogeneous_vector(int size);
void sk_local_parameterization_free(sk_local_parameterization* p);
int sk_local_parameterization_global_size(const sk_local_parameterization* p);  /* LocalParameterization::GlobalSize */
int sk_local_parameterization_local_size(const sk_local_parameterization* p);   /* LocalParameterization::LocalSize */
int sk_local_parameterization_plus(const sk_local_parameterization* p, const double* x, const double* delta, int n, double* x_plus);
int sk_local_parameterization_compute_jacobian(const sk_local_parameterization* p, const double* x, int n, double* jacobian);

/* ---- CostFunction -------------------------------------------------------- */
/* AutoDiffCostFunctor.toAutoDiffCostFunction (CORE/CostFunctor.scala:44) for a
 * functor with a device body.  Validates like CostFunctor / SizedCostFunction
 * (CORE/CostFunctor.scala:31-34, CORE/SizedCostFunction.scala:7-13).  Returns
 * NULL on an unknown id or wrong `num_consts`. */
sk_cost_function* sk_cost_function_new_autodiff(int functor_id, const double* consts, int num_consts);

/* Host-callback cost function: the reference's director path
 * ceres::CostFunction::Evaluate(double const* const* parameters,
 *   double* residuals, double** jacobians) -> bool   (ceres.i:48; overridden
 * at CORE/AutodiffCostFunction.scala:74-78).  `jacobians` may be NULL and each
 * jacobians[i] may be NULL; block i is row-major num_residuals x block_sizes[i].
 * Returns boolean (0 == evaluation failed). */
typedef int (*sk_evaluate_fn)(void* user, double const* const* parameters, double* residuals,
                              double** jacobians);
sk_cost_function* sk_cost_function_new_callback(sk_evaluate_fn fn, void* user, int num_residuals,
                                                const int* block_sizes, int num_blocks);
/* AutoDiffCostFunctor.toAutoDiffCostFunction (CORE/CostFunctor.scala:44) for a functor WITHOUT a device body: its
 * recorded body (see sk_tape_opcode).  `instructions`: 5 * num_instructions integers; `output_operands`: one operand per
 * residual; `captured`: the doubles this closure captures (num_captured of them; sk_problem_add_residual_blocks_tape
 * passes them per block instead).  Validates sizes as CostFunctor / SizedCostFunction do (CORE/CostFunctor.scala:31-34)
 * and every instruction (known opcode, operands in range, registers written before they are read).  NULL on error. */
sk_cost_function* sk_cost_function_new_tape(int num_residuals, const int* block_sizes, int num_blocks,
                                            const int* instructions, int num_instructions,
                                            const double* tape_constants, int num_tape_constants,
                                            int num_registers, const int* output_operands,
                                            const double* captured, int num_captured);
void sk_cost_function_free(sk_cost_function* cf);
int sk_cost_function_num_residuals(const sk_cost_function* cf);             /* CostFunction.numResiduals() */
int sk_cost_function_num_parameter_blocks(const sk_cost_function* cf);      /* parameterBlockSizes().size() */
int sk_cost_function_parameter_block_size(const sk_cost_function* cf, int i);
/* CostFunction.evaluate (CORE/AutodiffCostFunction.scala:74-134): evaluates ONE
 * residual block.  Device functors run on the GPU (one lane).  Boolean result;
 * a negative value is an error (see sk_last_error). */
int sk_cost_function_evaluate(const sk_cost_function* cf, double const* const* parameters,
                              double* residuals, double** jacobians);

/* ---- Problem: CeresProblem + CORE/Problem.scala --------------------------- */
sk_problem* sk_problem_new(void);                    /* new Problem (Options: never owns cost/loss) */
void sk_problem_free(sk_problem* p);
/* CeresProblem.addResidualBlock(CostFunction, LossFunction, StdVectorDoublePointer)
 * (CORE/Problem.scala:20-27; the only overload left by ceres.i:53-70).
 * Parameter blocks are identified BY POINTER VALUE; first sighting registers a
 * block of the size the cost function declares; a later sighting with another
 * size is SK_ERR_INVALID_ARGUMENT.  `loss` may be NULL (== trivial). */
int sk_problem_add_residual_block(sk_problem* p, const sk_cost_function* cost,
                                  const sk_loss_function* loss, double* const* parameter_blocks,
                                  int num_parameter_blocks, sk_residual_block_id* id_out);
/* Bulk form of the setup loop EX/SimpleBundleAdjuster.scala:139-145: adds
 * `n` residual blocks of one device functor in one call.  consts is
 * n x num_consts row-major; parameter_blocks is n x num_blocks row-major. */
int sk_problem_add_residual_blocks(sk_problem* p, int functor_id, int n, const double* consts,
                                   const sk_loss_function* loss, double* const* parameter_blocks);
/* The same for a recorded functor (sk_cost_function_new_tape): n residual blocks of the body of `cost`, block b with
 * the captured doubles captured[b * num_captured ..] (NULL when the body captures none). */
int sk_problem_add_residual_blocks_tape(sk_problem* p, const sk_cost_function* cost, int n, const double* captured,
                                        const sk_loss_function* loss, double* const* parameter_blocks);
/* Bulk add of `num_rows` residual blocks of a dense-row functor (SK_FUNCTOR_SYNTH_TANH_ROW) that all
 * depend on the single parameter block x[0..n).  consts is num_rows x 3 row-major.  `loss` (NULL == trivial) applies to
 * every row of the call; the dense-rows solver takes ONE loss for all rows of a problem (SK_ERR_UNSUPPORTED otherwise). */
int sk_problem_add_dense_rows(sk_problem* p, int functor_id, int num_rows, const double* consts,
                              const sk_loss_function* loss, double* x, int n);
/* ceres::Problem::AddParameterBlock(values, size[, local_parameterization]), SetParameterization,
 * SetParameterBlockConstant / SetParameterBlockVariable (inherited by CORE/Problem.scala:16 from the SWIG-wrapped
 * ceres::Problem).  `parameterization` may be NULL (none / remove).  The minimiser then works in the tangent
 * space: Jacobian columns J * dPlus/ddelta, steps applied through Plus; a constant block takes no step.
 * Implemented for DENSE_QR / DENSE_NORMAL_CHOLESKY over residual blocks (every type), and under DENSE_SCHUR for what
 * bundle adjustment uses: constant camera / point blocks, identity, and subset (e.g. fixed intrinsics on the 9-block) —
 * a coordinate that is held constant has a zero Jacobian column and takes no step.  sk_solve reports
 * SK_ERR_UNSUPPORTED for quaternion / homogeneous-vector blocks under DENSE_SCHUR and for dense-row problems. */
int sk_problem_add_parameter_block(sk_problem* p, double* values, int size, const sk_local_parameterization* parameterization);
int sk_problem_set_parameterization(sk_problem* p, double* values, const sk_local_parameterization* parameterization);
int sk_problem_set_parameter_block_constant(sk_problem* p, double* values);
int sk_problem_set_parameter_block_variable(sk_problem* p, double* values);
/* ceres::Problem::SetParameterLowerBound / SetParameterUpperBound and their getters (ceres/problem.h via ceres.i:150; inherited
 * by CORE/Problem.scala:16): coordinate `index` of the block at `values` stays inside [lower, upper].  A block that is not part
 * of the problem (by address), an index outside it and a NaN bound return SK_ERR_INVALID_ARGUMENT (the getters: NaN) with
 * sk_last_error; -/+ infinity removes a bound, and is what the getters return where nothing is set.
 *
 * The solve is Ceres 1.x's constrained trust-region loop, restated from memory like the rest of the minimiser (SURVEY.md
 * section 8a row a13; the constants: common.hpp, namespace bounds).  x is projected onto the box before the first evaluation
 * (initial_cost is the projected point's; it is written back even when no step is taken); gradient_max_norm is
 * max_j |x_j - P(x_j - g_j)|; the linear solve and the model's cost change are those of the unconstrained step delta; the
 * candidate is P(x + alpha delta), alpha from a backtracking Armijo line search on phi(alpha) = cost(P(x + alpha delta))
 * (sufficient decrease 1e-4, contraction inside [1e-3, 0.6] alpha, at most 20 contractions, minimum step 1e-9; alpha = 1 when it
 * fails or delta is no descent direction).  ONE DEPARTURE from Ceres' defaults: the next alpha is the minimiser of the quadratic
 * through (0, f0, slope g0) and (alpha, phi(alpha)) — function values only — where Ceres interpolates cubically with a Jacobian
 * at every trial point.  A variable block with lower >= upper at some index, or a constant block outside its bounds, makes
 * the problem infeasible: the solve ends with SK_FAILURE, the message names block and index, the parameters stay untouched.
 * Refused with SK_ERR_UNSUPPORTED when the solver is created: bounds with DOGLEG; in a world of more than one rank; on
 * dense-row problems; with host-evaluated (director) residual blocks under DENSE_SCHUR; on a block that carries a quaternion or
 * homogeneous-vector parameterization.  Constant blocks, identity and subset parameterizations and recorded functors are
 * taken.  Under bounds the iteration is enqueued launch by launch (sk_solver_stat "graph_replay" is 0); a problem without a
 * finite bound runs exactly what it ran before. */
int sk_problem_set_parameter_lower_bound(sk_problem* p, double* values, int index, double bound);
int sk_problem_set_parameter_upper_bound(sk_problem* p, double* values, int index, double bound);
double sk_problem_get_parameter_lower_bound(const sk_problem* p, const double* values, int index);
double sk_problem_get_parameter_upper_bound(const sk_problem* p, const double* values, int index);
int sk_problem_num_residual_blocks(const sk_problem* p);   /* Problem::NumResidualBlocks */
int sk_problem_num_parameter_blocks(const sk_problem* p);  /* Problem::NumParameterBlocks */
int sk_problem_num_parameters(const sk_problem* p);        /* Problem::NumParameters */
/* (no reference counterpart) the index of a parameter block in the problem's own order — the order of first mention, which the
 * *_of_block arrays of the plan functions below follow —, or -1 when values is no parameter block of the problem */
int sk_problem_parameter_block_index(const sk_problem* p, const double* values);
int sk_problem_num_residuals(const sk_problem* p);         /* Problem::NumResiduals */

/* ---- Problem::Evaluate: ceres::Problem::Evaluate(EvaluateOptions, cost, residuals, gradient, CRSMatrix*) -----------------
 * ceres/problem.h and ceres/crs_matrix.h, both %include'd by ceres.i; inherited by CORE/Problem.scala:16.  Cost, residuals,
 * gradient and the Jacobian in compressed-row form at the CURRENT contents of the caller's parameter memory (bounds play no part).
 * The semantics are Ceres 1.x's, restated from memory like the rest of the minimiser:
 *   rows      the residual blocks of the list, in list order (no list: in the order added), num_residuals rows each — whatever
 *             order the kernels evaluate them in;
 *   columns   the parameter blocks of the list, in list order (no list: in the order first seen), each with its tangent size: the
 *             local size of its parameterization, else its size.  A block absent from a given list is held constant for the call and
 *             has no columns.  A block that is constant (sk_problem_set_parameter_block_constant) and listed (or present, with no
 *             list) KEEPS its columns but has no stored entries and a zero gradient — unlike the solvers, whose internal convention
 *             is local size 0 for a constant block;
 *   loss      apply_loss_function on (the default) and a block with a loss: cost = 1/2 sum rho(|r_b|^2), residuals and Jacobian
 *             corrected as the solvers' corrector does it (residuals whenever they are asked for); off, or no loss: the plain r, J
 *             and 1/2 sum |r|^2;
 *   Jacobian  per residual block and non-constant parameter block the dense num_residuals x tangent size block
 *             J_global * dPlus/ddelta (subset: a column selection), every entry stored, zeros included; within a row the columns
 *             ascend strictly, so a residual block whose parameter blocks are not in column order has its blocks permuted.  rows /
 *             cols are 32-bit as in ceres::CRSMatrix: a matrix with 2^31 entries or more is SK_ERR_UNSUPPORTED;
 *   gradient  J^T r of exactly that matrix and those residuals (so it follows apply_loss_function), summed in a fixed order:
 *             two calls on the same inputs return the same bytes.
 * Device functors, recorded functors and host-callback blocks (evaluated on the host through their sk_evaluate_fn) are all taken;
 * nothing depends on a linear solver type, a block shape or a world of ranks: one device.  EvaluateOptions::num_threads has no
 * counterpart.  Errors: SK_ERR_INVALID_ARGUMENT — an id out of range or listed twice, a pointer that is no parameter block of the
 * problem or is listed twice; SK_ERR_NO_DEVICE — sk_problem_evaluate without a GPU (the two host-only calls need none);
 * SK_ERR_EVALUATION_FAILED — a functor or callback reported failure (outputs unspecified); SK_ERR_UNSUPPORTED — a problem with
 * dense rows (sk_problem_add_dense_rows), whose Jacobian is dense by construction. */
typedef struct sk_evaluate_options sk_evaluate_options;      /* ceres::Problem::EvaluateOptions */
sk_evaluate_options* sk_evaluate_options_new(void);          /* all parameter blocks, all residual blocks, apply_loss_function = 1, current device */
void sk_evaluate_options_free(sk_evaluate_options* o);
int sk_evaluate_options_set_apply_loss_function(sk_evaluate_options* o, int on);
int sk_evaluate_options_set_residual_blocks(sk_evaluate_options* o, const sk_residual_block_id* ids, int n);   /* n == 0: all, in the order added */
int sk_evaluate_options_set_parameter_blocks(sk_evaluate_options* o, double* const* blocks, int n);           /* n == 0: all, in the order first seen */
int sk_evaluate_options_set_device(sk_evaluate_options* o, int hip_device);
/* (no reference counterpart) on != 0: sk_problem_evaluate records HIP events around its phases, and _launch_seconds returns the
 * device seconds of the last call's phase: 0 uploads, 1 evaluation launches (with the host callbacks), 2 finish, 3 gradient,
 * 4 cost, 5 downloads. */
int sk_evaluate_options_set_launch_timing(sk_evaluate_options* o, int on);
double sk_evaluate_options_launch_seconds(const sk_evaluate_options* o, int phase);
/* host data alone, no device needed */
int sk_problem_evaluate_sizes(const sk_problem* p, const sk_evaluate_options* o, int* num_rows, int* num_cols, long long* num_nonzeros);
int sk_problem_evaluate_structure(const sk_problem* p, const sk_evaluate_options* o, int* rows /* num_rows + 1 */, int* cols /* num_nonzeros */);
/* on the device; every output may be NULL; o may be NULL (defaults) */
int sk_problem_evaluate(sk_problem* p, const sk_evaluate_options* o, double* cost, double* residuals /* num_rows */,
                        double* gradient /* num_cols */, double* jacobian_values /* num_nonzeros */);

/* ---- Covariance: ceres::Covariance and ceres::Covariance::Options ------------------------------------------------------------
 * ceres/covariance.h, #include'd at ceres.i:29 and %include'd at ceres.i:141: both are classes of the JVM module that bindings/
 * replaces.  The semantics are Ceres 1.x's, restated from memory like the rest:
 *   C = (J^T J)^-1 with J the Jacobian sk_problem_evaluate would return at the CURRENT contents of the caller's parameter memory,
 *   over all residual blocks and all parameter blocks, in the tangent space, loss-corrected iff apply_loss_function.
 *   sizes      a block (a, b) is served in the tangent space, tangent(a) x tangent(b), or lifted to the ambient space,
 *              P_a C_ab P_b^T, size(a) x size(b), with P = dPlus/ddelta at the current x (subset: zero rows and columns at the held
 *              coordinates; quaternion: 4 x 4 of rank 3); both row-major;
 *   constant   a constant block has covariance zero with everything, itself included; its tangent size is Problem::Evaluate's
 *              (the local size of its parameterization, else its size);
 *   algorithm  the Cholesky factorisation of the diagonally scaled normal matrix D J^T J D, dense, on the device (the conditioning
 *              caveat of the normal equations applies: kappa(J^T J) = kappa(J)^2).  A rank-deficient Jacobian makes compute FAIL:
 *              Ceres' DENSE_SVD pseudo-inverse, null_space_rank and algorithm_type have no counterpart.  Rank deficiency is decided
 *              by (1) a diagonal entry of J^T J that is exactly 0 (a coordinate no residual depends on, a block in no residual
 *              block) and (2) a pivot that is not positive, or min_j L_jj^2 / max_j L_jj^2 < min_reciprocal_condition_number;
 *   pairs      (a, b) and (b, a) are one pair; duplicates are accepted and computed once; the getters answer both orders:
 *              block(b, a) is block(a, b) transposed, bit for bit.
 * Errors: SK_ERR_INVALID_ARGUMENT — a pointer that is no parameter block of the problem, num_pairs <= 0, a getter before a
 * successful compute or for a pair that was not computed (get_matrix: any pair among the listed blocks); SK_ERR_NO_DEVICE —
 * compute without a GPU (options, getters and validation need none); SK_ERR_EVALUATION_FAILED — a functor reported failure, or
 * the Jacobian is rank deficient (sk_last_error names the first offending block and coordinate, else the pivot ratio; getters
 * afterwards are SK_ERR_INVALID_ARGUMENT); SK_ERR_UNSUPPORTED — dense-row problems, a tangent size above 16, more than 32 768
 * columns (the dense matrix of (N + k, padded to blocks of 128)^2 doubles is a cap on memory; covariance at bundle-adjustment scale
 * takes the Schur elimination below).  Host-callback blocks are taken; one device, no world of ranks.
 *   Schur elimination (sk_covariance_options_set_schur_elimination, off by default: then the route above, byte for byte).  With it
 *              an independent set E of the moving blocks is eliminated block by block in front of the dense factorisation, and the
 *              eliminated blocks are substituted back behind it: H = [[U, W], [W^T, V]], V block diagonal over E, H~ = D H D with D
 *              over all columns, per e-block V~_e = L_e L_e^T and X_ge = D_g W_ge D_e L_e^-T, S~ = U~ - sum_e X_ge X_g'e^T factored
 *              densely with the selection as its border.  E is greedy: two blocks are neighbours when a residual block stores both;
 *              the moving blocks are visited in ascending order of (number of distinct neighbours, parameter-block index) and a
 *              block joins E when none of its neighbours is in E yet; the rest, F, keeps the problem's order.  E depends on the
 *              problem alone (bundle adjustment: the points; a block in no residual block joins first and is reported as above).
 *              A requested e-block adds all its F-neighbours to the selection ("selected_columns" counts them).  Every problem
 *              the dense route takes in kind is taken; SK_ERR_UNSUPPORTED from host data alone: dense rows, a tangent size above
 *              16, more than 32 768 columns left AFTER the elimination, more than 2^31 - 1 Schur terms.  Two computes return the
 *              same bytes; the two routes agree to rounding, not bitwise.
 *   min_reciprocal_condition_number  is compared with min L_jj^2 / max L_jj^2 of the Cholesky factor of H~.  With the Schur
 *              elimination that is the factor of H~ WITH E ORDERED FIRST (the pivots of every L_e and of S~'s factor), so the value
 *              differs from the dense route's on the same problem; the rule and its messages are otherwise the same. */
typedef struct sk_covariance_options sk_covariance_options;   /* ceres::Covariance::Options (ceres/covariance.h via ceres.i:29,141) */
typedef struct sk_covariance sk_covariance;                   /* ceres::Covariance (ceres/covariance.h via ceres.i:29,141) */
sk_covariance_options* sk_covariance_options_new(void);       /* apply_loss_function 1, min_reciprocal_condition_number 1e-14, current device */
void sk_covariance_options_free(sk_covariance_options* o);
int sk_covariance_options_set_apply_loss_function(sk_covariance_options* o, int on);                  /* Covariance::Options::apply_loss_function */
int sk_covariance_options_set_min_reciprocal_condition_number(sk_covariance_options* o, double v);    /* Covariance::Options::min_reciprocal_condition_number; [0, 1), not NaN */
int sk_covariance_options_set_device(sk_covariance_options* o, int hip_device);                       /* (no reference counterpart) */
int sk_covariance_options_set_schur_elimination(sk_covariance_options* o, int on);                    /* (no reference counterpart) default 0: see above */
/* (no reference counterpart) the eliminated set of the Schur elimination, from host data alone (no device): eliminated_of_block
 * [parameter blocks], may be NULL: 1 in E, 0 in F, -1 constant / no columns; the number of blocks in E, the columns of the reduced
 * matrix and the number of Schur terms (any may be NULL).  SK_ERR_UNSUPPORTED as a compute with the option on. */
int sk_covariance_elimination_plan(const sk_problem* p, int* eliminated_of_block, int* num_eliminated, int* reduced_columns, long long* schur_terms);
sk_covariance* sk_covariance_new(const sk_covariance_options* o /* may be NULL */);                   /* Covariance::Covariance(options) */
void sk_covariance_free(sk_covariance* c);
/* Covariance::Compute(covariance_blocks, problem): the pairs (blocks1[i], blocks2[i]) */
int sk_covariance_compute(sk_covariance* c, sk_problem* p, double* const* blocks1, double* const* blocks2, int num_pairs);
/* Covariance::Compute(parameter_blocks, problem): every pair among the n blocks — the form a StdVectorDoublePointer (ceres.i:82) can carry */
int sk_covariance_compute_blocks(sk_covariance* c, sk_problem* p, double* const* blocks, int n);
int sk_covariance_get_block(const sk_covariance* c, const double* b1, const double* b2, double* out);                   /* Covariance::GetCovarianceBlock: size(b1) x size(b2) */
int sk_covariance_get_block_in_tangent_space(const sk_covariance* c, const double* b1, const double* b2, double* out);  /* Covariance::GetCovarianceBlockInTangentSpace */
int sk_covariance_get_matrix(const sk_covariance* c, double* const* blocks, int n, double* out);                        /* Covariance::GetCovarianceMatrix: (sum sizes)^2, listed order */
int sk_covariance_get_matrix_in_tangent_space(const sk_covariance* c, double* const* blocks, int n, double* out);       /* Covariance::GetCovarianceMatrixInTangentSpace */
/* (no reference counterpart) of the last compute: "columns" (N), "selected_columns" (k), "normal_matrix_pairs",
 * "reciprocal_pivot_ratio", "schur_elimination" (0 or 1), "eliminated_blocks", "reduced_columns" (N without the elimination),
 * "schur_terms", "phase_seconds_0".."phase_seconds_4" — device seconds from HIP events: 0 evaluation, 1 assembly and
 * scaling (with the elimination: up to and including the Schur update), 2 factorisation, 3 extraction, 4 downloads.  SK_ERR_INVALID_ARGUMENT for another name or before a compute reached the device. */
int sk_covariance_stat(const sk_covariance* c, const char* name, double* value);
/* (no reference counterpart) what a binding sizes its arrays by: the size and the tangent size of a parameter block of the problem
 * of the last successful compute (either pointer may be NULL).  SK_ERR_INVALID_ARGUMENT as for the getters. */
int sk_covariance_block_sizes(const sk_covariance* c, const double* block, int* size, int* tangent_size);

/* ---- Solver.Options (setters are ceres.i:89-92 lowerCamelCase renames) ---- */
sk_options* sk_options_new(void);                    /* Ceres 1.x defaults, SURVEY.md §8a row a13 */
void sk_options_free(sk_options* o);
int sk_options_set_linear_solver_type(sk_options* o, int type);       /* setLinearSolverType */
int sk_options_set_minimizer_type(sk_options* o, int type);           /* setMinimizerType; TRUST_REGION only */
int sk_options_set_max_num_iterations(sk_options* o, int n);          /* setMaxNumIterations */
int sk_options_set_minimizer_progress_to_stdout(sk_options* o, int on); /* setMinimizerProgressToStdout */
int sk_options_set_function_tolerance(sk_options* o, double v);
int sk_options_set_gradient_tolerance(sk_options* o, double v);
int sk_options_set_parameter_tolerance(sk_options* o, double v);
int sk_options_set_initial_trust_region_radius(sk_options* o, double v);
int sk_options_set_max_trust_region_radius(sk_options* o, double v);
int sk_options_set_min_trust_region_radius(sk_options* o, double v);
int sk_options_set_min_relative_decrease(sk_options* o, double v);
int sk_options_set_min_lm_diagonal(sk_options* o, double v);
int sk_options_set_max_lm_diagonal(sk_options* o, double v);
int sk_options_set_jacobi_scaling(sk_options* o, int on);
int sk_options_set_max_num_consecutive_invalid_steps(sk_options* o, int n);
/* CGNR (linear solver type SK_CGNR): every trust-region step is an inexact Newton step — preconditioned conjugate gradients on
 * (J^T J + D^2) y = -J^T r, the matrix applied as two products with the block-sparse Jacobian and never formed (Ceres 1.x's
 * ConjugateGradientsSolver: stop when it * (Q_it - Q_it-1) / Q_it < eta and it >= min_linear_solver_iterations, or at
 * max_linear_solver_iterations, whose step is used; the residual is formed anew as b - A x every tenth iteration).  Defaults:
 * JACOBI (the block diagonal of the matrix over the parameter blocks), eta 0.1, at most 500 and at least 0 iterations.
 * SK_ERR_INVALID_ARGUMENT: a preconditioner type other than the two, eta outside (0, 1), a negative count, min > max.
 * Taken: device functors and recorded functors, robust losses, constant blocks, the four local parameterizations,
 * bundle-adjustment-shaped problems (as the full camera + point system, or with sk_options_set_schur_elimination on the
 * reduced camera system).  Refused with SK_ERR_UNSUPPORTED when the solver is
 * created: host-evaluated (director) residual blocks, a parameter block of tangent size above 16, DOGLEG, parameter bounds, a
 * world of more than one rank, dense-row problems.  sk_options_set_cholesky_tuning has no effect.  The iteration is enqueued
 * launch by launch (sk_solver_stat "graph_replay" is 0); the step does not depend on how many CG iterations are enqueued
 * between two reads of the device's done flag. */
int sk_options_set_preconditioner_type(sk_options* o, int type);
int sk_options_set_eta(sk_options* o, double eta);
int sk_options_set_max_linear_solver_iterations(sk_options* o, int n);
int sk_options_set_min_linear_solver_iterations(sk_options* o, int n);
/* (no reference counterpart) CGNR on the implicit Schur complement.  Default 0.  on != 0, under SK_CGNR only (no effect under the
 * other solver types): an independent set E of the moving parameter blocks is eliminated (the greedy rule of
 * sk_covariance_options_set_schur_elimination: a bundle-adjustment problem's points), and the same conjugate-gradient loop solves
 * S y_F = s with S = U - W V^-1 W^T over the kept blocks F, applied as S v = J_F^T (I - J_E V^-1 J_E^T) J_F v + D_F^2 v and never
 * formed; then y_E = V^-1 (b_E - W^T y_F).  SK_JACOBI is then the block diagonal of S (Ceres' SCHUR_JACOBI), SK_IDENTITY none.
 * When every moving block is in E the step is the back-substitution alone: 0 CG iterations, status 0.  Accepts and refuses what
 * CGNR does.  sk_solver_stat: "schur_elimination" (0 or 1), "eliminated_blocks", "reduced_columns" (the columns CG runs on),
 * "schur_diagonal_pairs" (the (F block, e-block) pairs that the block diagonal of S sums over); the full report names the
 * elimination and the two counts when the option is on. */
int sk_options_set_schur_elimination(sk_options* o, int on);
/* (no reference counterpart) the elimination of sk_options_set_schur_elimination for this problem, from host data alone (no
 * device): eliminated_of_block [parameter blocks]: 1 in E, 0 in F, -1 constant / no columns; the number of blocks in E, the columns
 * of F, the e-blocks on more than 64 residual blocks (summed in two launches) and the (F block, e-block) pairs.  Any pointer may be
 * NULL.  SK_ERR_UNSUPPORTED as a CGNR solver on one rank with LEVENBERG_MARQUARDT refuses the problem. */
int sk_cgnr_elimination_plan(const sk_problem* p, int* eliminated_of_block, int* num_eliminated, int* reduced_columns, int* long_eliminated_blocks, int* fe_pairs);
/* Inner iterations (Solver::Options::use_inner_iterations, inner_iteration_tolerance, inner_iteration_ordering; Ceres 1.x,
 * restated from memory).  Default off; under SK_CGNR only, with or without sk_options_set_schur_elimination: every other linear
 * solver type makes sk_solver_create return SK_ERR_UNSUPPORTED with a message that names the solver.  After every trust-region
 * step that is valid and has a positive model cost change, each parameter block of an independent set (group 0) is minimised on
 * its own, all the others held, then group 1 follows, and so on.  One such solve is the Levenberg-Marquardt loop of this library
 * with Ceres' default options (50 iterations, function tolerance 1e-6, gradient tolerance 1e-10, parameter tolerance 1e-8,
 * initial radius 1e4), not the outer solve's; its linear solve is a Cholesky factorisation of the block's damped normal matrix
 * (Ceres: DENSE_QR).  With c the current cost, c_tr the candidate's and c_in the refined candidate's: model_cost_change += c_tr -
 * c_in; the step is successful when rho > min_relative_decrease or c_in < c; the refinement switches itself off for the rest of
 * the solve once 1 - c_in / c_tr <= inner_iteration_tolerance (default 1e-3; >= 0).
 * Ordering: n = 0 (the default) is automatic — group 0 the greedy independent set of sk_options_set_schur_elimination on the moving
 * blocks, group k the same rule on the blocks still ungrouped with their neighbours counted among those alone (bundle adjustment:
 * the points, then the cameras).  n > 0: blocks[i] is refined in group groups[i] (ascending ids; >= 0); unlisted blocks are not
 * refined and constant blocks are ignored.  The pointers are copied, not the memory.  sk_solver_create returns
 * SK_ERR_INVALID_ARGUMENT for a pointer that is no parameter block of the problem and for a group that is not an independent
 * set (the message names the two blocks that a residual block joins). */
int sk_options_set_use_inner_iterations(sk_options* o, int on);
int sk_options_get_use_inner_iterations(const sk_options* o);
int sk_options_set_inner_iteration_tolerance(sk_options* o, double v);
double sk_options_get_inner_iteration_tolerance(const sk_options* o);
int sk_options_set_inner_iteration_ordering(sk_options* o, double* const* blocks, const int* groups, int n);
/* (no reference counterpart) the groups of the options' ordering (o == NULL: automatic) for this problem, from host data alone
 * (no device): group_of_block [parameter blocks]: the group, -1 not refined; the number of groups.  Any output may be NULL.
 * SK_ERR_UNSUPPORTED as a CGNR solver refuses the problem, SK_ERR_INVALID_ARGUMENT as sk_solver_create refuses the ordering. */
int sk_inner_iteration_plan(const sk_problem* p, const sk_options* o, int* group_of_block, int* num_groups);
/* MI355X-side knobs (no reference counterpart) */
int sk_options_set_device(sk_options* o, int hip_device);             /* default: current device */
int sk_options_set_stream(sk_options* o, void* hip_stream);           /* default: a private stream */
/* Tuning of the dense Cholesky: `group` = depth of the trailing SYRK in 128-column blocks (K = 128*group).
 * <= 0 (default) leaves the plan to the library: groups of 3 for a full factorisation; with a sparse block
 * envelope, groups of 2 where the trailing SYRK is the long pole and single columns under a resident panel chain
 * (one workgroup that factors the diagonal blocks, per-column launches that hand it its operands through device
 * counters) where the serial chain is — DESIGN.md section 4.  The first solver of a process then spends about
 * 0.1 s choosing hardware queues for that chain.  An explicit `group` is used for every column, launch by launch
 * (then the envelope factorisation is bit-identical to the full one at the same `group`).
 * `lookahead` != 0 factors the next block-column group on its own stream next to the trailing SYRK of the
 * current one. */
int sk_options_set_cholesky_tuning(sk_options* o, int group, int lookahead);
/* DENSE_SCHUR: the reduced camera system of a bundle-adjustment problem is block-banded (cameras that share no
 * point give a zero block, and the Cholesky factor keeps the block envelope).  on != 0 (default): the dense
 * factorisation touches only the 128-blocks inside the envelope; the blocks it leaves out are exact zeros in the
 * full computation too, so at equal SYRK depth (sk_options_set_cholesky_tuning) the result is bit-identical to
 * on == 0, which factors every block. */
int sk_options_set_cholesky_envelope(sk_options* o, int on);
/* DENSE_SCHUR: two-way dissection of the camera sequence.  The block-banded reduced system of a camera sequence is a
 * serial chain of one 128-block column after the other; the cameras are split into a head, a separator and a tail (no
 * point seen from both head and tail), the head is eliminated front to back and the tail back to front, side by side
 * on two sets of queues, and the separator's system — plus both Schur complements — is factored last: the same
 * arithmetic in another elimination order (results agree with the undissected factorisation to rounding, not bit for
 * bit), with a chain about half as long.  ON: whenever a separator exists, with the library's own plan (no explicit
 * `group`), the envelope on and one process; OFF: never; AUTO (default): as OFF on one device — measured on MI355X the
 * two chains disturb each other on one chip more than the shorter chain gains — the model's
 * prediction is reported by sk_solver_stat. */
enum { SK_DISSECTION_AUTO = 0, SK_DISSECTION_ON = 1, SK_DISSECTION_OFF = 2 };
int sk_options_set_cholesky_dissection(sk_options* o, int mode);
/* DENSE_SCHUR: loop closures.  A camera sequence that revisits a place couples two distant windows of the band, and in
 * the band's own order every block column between the two windows joins the envelope.  The solver may instead number
 * the revisiting cameras BEHIND the band, as a border whose block rows are active from the first block column that
 * reaches them (and whose own block columns are factored last): the band keeps its width.  The result of the solve
 * does not depend on the order of the cameras inside the reduced system (Ceres' DENSE_SCHUR,
 * examples/.../SimpleBundleAdjuster.scala:147-152, orders it itself); another elimination order agrees to rounding,
 * not bit for bit.  AUTO (default): when the model of the factorisation's serial chain predicts a gain of 10 %;
 * ON: whenever the camera lists of the points show visits (jumps in the camera sequence) — tests, small problems;
 * OFF: never.  sk_solver_stat: "border_cameras", "border_gap", "border_model_us", "border_model_us_plain". */
/* Resident kernels.  By default the factorisation of the reduced system runs its chain-bound block columns under a RESIDENT
 * panel chain (one workgroup that factors the diagonal blocks as their updates land, column launches enqueued ahead of time
 * that wait for it) and the back-substitution is one resident launch — kernels that wait for other kernels of the same
 * process.  on == 0: this solver uses none — the same factorisation plan and the same arithmetic, one launch per step —
 * for processes in which kernels are serialised (hardware-counter collection under rocprofv3 --pmc) or in which the caller
 * does not want kernels that spin.  (A wait that gives up after its 1 s time-out has the same effect for the device from
 * then on, and says so on stderr.) */
int sk_options_set_resident_kernels(sk_options* o, int on);
/* Launch-bound problems (a reduced system of at most eight 128-blocks: BAL problem-49) replay their iteration as a hipGraph;
 * on == 0: every launch is enqueued directly. */
int sk_options_set_graph_replay(sk_options* o, int on);
/* Several ranks, SK_DISTRIBUTION_SEGMENTED / AUTO: cut the camera sequence into at most n segments (0, the default: at
 * most one per rank; n >= 2 otherwise). */
int sk_options_set_max_segments(sk_options* o, int n);
/* Solver::Options::trust_region_strategy_type / dogleg_type (ceres/types.h via ceres.i:137; ceres/solver.h via ceres.i:151).
 * LEVENBERG_MARQUARDT is the default.  DOGLEG (TRADITIONAL) follows Ceres 1.x's DoglegStrategy: the Gauss-Newton step and the
 * Cauchy point depend on the Jacobian alone, so a rejected step is followed by a re-interpolation of the two vectors at half
 * the radius — no assembly, no factorisation (sk_solver_stat "dogleg_reused_steps").  An out-of-range value returns
 * SK_ERR_INVALID_ARGUMENT.  Refused with SK_ERR_UNSUPPORTED when the solver is created (sk_solver_create / sk_solve):
 * SK_SUBSPACE_DOGLEG; DOGLEG in a world of more than one rank; DOGLEG on dense-row problems; and the two combinations that are
 * not carried through: DOGLEG with tangent-space blocks (local parameterizations, constant blocks) on the dense Jacobian path
 * (DENSE_QR / DENSE_NORMAL_CHOLESKY over residual blocks; DENSE_SCHUR takes constant blocks and subsets), and DOGLEG with
 * host-evaluated (director) residual blocks under DENSE_SCHUR (the dense path takes them).  Under DOGLEG the iteration is
 * enqueued launch by launch (sk_solver_stat "graph_replay" is 0). */
int sk_options_set_trust_region_strategy_type(sk_options* o, int type);
int sk_options_set_dogleg_type(sk_options* o, int type);
/* The two fields read back, as a caller of the reference reads options.trust_region_strategy_type (a public field of
 * Solver::Options, ceres/solver.h via ceres.i:151): what the setters left; the defaults are LEVENBERG_MARQUARDT and
 * TRADITIONAL_DOGLEG. */
int sk_options_get_trust_region_strategy_type(const sk_options* o);
int sk_options_get_dogleg_type(const sk_options* o);
enum { SK_BORDER_AUTO = 0, SK_BORDER_ON = 1, SK_BORDER_OFF = 2 };
int sk_options_set_cholesky_border(sk_options* o, int mode);
/* DENSE_SCHUR: RETAINED POINTS.  The Schur complement of a point seen by k cameras is a dense k x k square of camera blocks; a
 * landmark that stays in view for hundreds of frames sets the height of the reduced system's block envelope over every block
 * column it spans (the Ladybug-1723-shaped problem: 5 of 156 502 points account for 80 % of the factorisation's flops).  Such
 * points are not eliminated: their three coordinates stay in the reduced system as three more rows behind the cameras — a
 * border in the sense of sk_options_set_cholesky_border — and the Schur complement is formed from the other points alone.  The
 * linear system, and therefore the LM step, is the same (Ceres' DENSE_SCHUR eliminates every point,
 * examples/.../SimpleBundleAdjuster.scala:147-152; which unknowns are eliminated first changes rounding only).  AUTO (default):
 * the widest tracks, as many as the model of the factorisation's serial chain says pay, when it predicts 10 % less than
 * eliminating everything; ON: the best count whatever the model says (tests, small problems); OFF: every point is eliminated.
 * max_points: at most this many — with ON: exactly this many, as far as there are tracks wider than a block — (a multiple of three is
 * used; 0: the library's limit, 1536).  Candidates: the widest tracks by span and by number of observations, and the tracks of
 * loop closures (a jump in the point's camera list) at their exact number.  A point with two residual blocks on one camera is never
 * retained.  Several ranks: the SEGMENTED distribution takes them with any number of segments — cut in two, the pseudo-cameras are
 * members of the one separator; cut in more, a border of the root and of every segment's front (AUTO tries two segments first and more
 * where its model says so; sk_options_set_max_segments caps the number) — and a retained point's observations are split over the
 * ranks by camera.  sk_solver_stat: "retained_points", "retained_model_us", "retained_model_us_without",
 * "model_us_two_segments_with_members". */
enum { SK_RETAINED_AUTO = 0, SK_RETAINED_ON = 1, SK_RETAINED_OFF = 2 };
int sk_options_set_retained_points(sk_options* o, int mode, int max_points);
/* Multi-GPU: this process is rank `rank` of `world` ranks,
 * one per GPU.  Points (e-blocks) are partitioned over ranks; the
 * normal-equation terms are summed with `allreduce` once per linear solve.
 * The hook must sum `count` doubles in device memory in place across all
 * ranks, ordered after prior work on `hip_stream`, and return 0.  It may return as soon as the collective is ENQUEUED on
 * `hip_stream` (the solver goes on enqueueing behind it and synchronises only where it reads a result: no host
 * synchronisation follows the hook since round 5); a hook that stages through the host synchronises the stream itself. */
typedef int (*sk_allreduce_fn)(void* user, double* device_buffer, size_t count, void* hip_stream);
int sk_options_set_distributed(sk_options* o, int rank, int world, sk_allreduce_fn allreduce,
                               void* user);
/* A ready-made `allreduce` over RCCL for callers that have no collective of their own (C, C++, the JVM: INTEGRATION.md
 * section 3) — the native counterpart of skeres_amd/dist.py's torch.distributed hook.  librccl.so is opened at run time
 * (dlopen): the library loads without it, and these calls then fail with SK_ERR_COMM / NULL + sk_last_error.
 *   rank 0:      sk_rccl_unique_id(id)  — 128 bytes (ncclUniqueId), passed to the other ranks by the caller's own means;
 *   every rank:  h = sk_allreduce_rccl_init(rank, world, id)  — ncclCommInitRank on the CURRENT HIP device — or
 *                h = sk_allreduce_rccl_create(comm) around an ncclComm_t the caller already has (not destroyed by _free);
 *                sk_options_set_distributed(o, rank, world, sk_allreduce_rccl_fn(), h);
 *   afterwards:  sk_allreduce_rccl_free(h).
 * The hook is an in-place ncclAllReduce(ncclDouble, ncclSum) on the stream the solver hands it. */
typedef struct sk_rccl sk_rccl;
int sk_rccl_unique_id(void* id128);
sk_rccl* sk_allreduce_rccl_init(int rank, int world, const void* id128);
sk_rccl* sk_allreduce_rccl_create(void* nccl_comm);
void sk_allreduce_rccl_free(sk_rccl* h);
long sk_allreduce_rccl_calls(const sk_rccl* h);
sk_allreduce_fn sk_allreduce_rccl_fn(void);
/* SEGMENTED: the camera sequence is dissected (sk_options_set_cholesky_dissection): rank 0's device eliminates the head and
 * its points, rank 1's the tail (further ranks replicate rank r mod 2 and add zeros to the sums); what is all-reduced per
 * iteration is the separator's system with both Schur complements — a few MB instead of the reduced system — and the two
 * serial chains run on two chips.  Chosen by AUTO when the model of the two chains predicts a gain; asked for explicitly it
 * is SK_ERR_UNSUPPORTED for a problem without a separator or with an explicit Cholesky grouping.
 * What a world > 1 does with its ranks.  SHARDED: points partitioned, one all-reduce of the reduced system
 * (its lower block triangle, packed) per linear solve.  REPLICATED: every rank solves the whole problem, no
 * collective.  AUTO (default): the solver times the all-reduce on the real buffer at set-up, estimates the
 * per-iteration work sharding would remove, and shards only when that pays (same decision on every rank). */
enum { SK_DISTRIBUTION_AUTO = 0, SK_DISTRIBUTION_SHARDED = 1, SK_DISTRIBUTION_REPLICATED = 2, SK_DISTRIBUTION_SEGMENTED = 3 };
int sk_options_set_distribution_mode(sk_options* o, int mode);
/* The caller may hand the solver the buffer the big all-reduce runs on (so a
 * torch.distributed / RCCL communicator can register it).  bytes must be >=
 * sk_reduce_buffer_bytes(problem, options): the whole lower block triangle, an upper bound — the solver packs and
 * reduces only the blocks inside the envelope (sk_solver_stat "allreduce_bytes"), at the start of the buffer. */
int sk_options_set_reduce_buffer(sk_options* o, void* device_ptr, size_t bytes);
size_t sk_reduce_buffer_bytes(const sk_options* o, const sk_problem* p);

/* ---- Solver.Summary ------------------------------------------------------- */
sk_summary* sk_summary_new(void);
void sk_summary_free(sk_summary* s);
double sk_summary_initial_cost(const sk_summary* s);
double sk_summary_final_cost(const sk_summary* s);
int sk_summary_num_iterations(const sk_summary* s);          /* iterations incl. iteration 0, as Ceres counts */
int sk_summary_num_successful_steps(const sk_summary* s);
int sk_summary_num_unsuccessful_steps(const sk_summary* s);
int sk_summary_termination_type(const sk_summary* s);
const char* sk_summary_message(const sk_summary* s);
const char* sk_summary_brief_report(const sk_summary* s);    /* Summary.briefReport(); EX/CurveFitting.scala:131 */
const char* sk_summary_full_report(const sk_summary* s);     /* Summary.fullReport(); EX/SimpleBundleAdjuster.scala:154 */
/* Per-iteration log (what minimizer_progress_to_stdout prints). field:
 * 0 cost, 1 cost_change, 2 gradient_max_norm, 3 step_norm, 4 relative_decrease,
 * 5 trust_region_radius, 6 step_is_valid, 7 step_is_successful,
 * 8 step_size (the line search's alpha under parameter bounds; 1 without), 9 line_search_evaluations (candidate costs
 * evaluated in the iteration: the ls_iter column; 1 without bounds), 10 linear_solver_iterations (CGNR: the CG iterations of
 * the iteration's linear solve; 0 for the factorisation solvers), 11 inner_iteration_rounds (use_inner_iterations: the
 * lock-step rounds that refined the iteration's candidate; 0 when it was not refined) */
int sk_summary_num_logged_iterations(const sk_summary* s);
double sk_summary_iteration_field(const sk_summary* s, int iteration, int field);
/* Device time per phase, seconds, summed over the solve (HIP events on the
 * solver's stream). phase: 0 jacobian_eval, 1 schur_assemble (or J^T J),
 * 2 cholesky (or QR), 3 back_substitute, 4 cost_eval, 5 allreduce, 6 total.
 * CGNR: 1 the block sums and the preconditioner, 2 the CG loop, 3 the model and the candidate */
double sk_summary_phase_seconds(const sk_summary* s, int phase);
/* Summary.linear_solver_type_used / _given (ceres::Solver::Summary; SWIG exposes both through /root/reference ceres.i:186-210).
   They differ when DENSE_SCHUR was asked for on a problem without the 2-residual / 9- and 3-parameter block structure: the
   alternate, DENSE_QR, is used, as Ceres does for a Schur-type solver with nothing to eliminate. */
int sk_summary_linear_solver_type_used(const sk_summary* s);
int sk_summary_linear_solver_type_given(const sk_summary* s);

/* ---- solve ----------------------------------------------------------------- */
/* ceres.solve(options, problem, summary) — EX/SimpleBundleAdjuster.scala:152,
 * EX/CurveFitting.scala:127.  Blocking; parameters updated in place. */
int sk_solve(const sk_options* options, sk_problem* problem, sk_summary* summary);

/* Stepping form of the same loop, for benchmarks and JVM IterationCallback-style
 * drivers: create (uploads + iteration 0), step (ONE trust-region iteration),
 * finish (writes parameters back + fills the summary). */
sk_solver* sk_solver_create(const sk_options* options, sk_problem* problem);
/* The sk_status that goes with the last NULL returned by sk_solver_create — or by sk_allreduce_rccl_init — on the calling thread
 * (SK_OK after a success; both set it on every call): NULL alone cannot say whether the device is missing, the configuration
 * unsupported, the communicator down or an argument wrong. */
int sk_last_status(void);
void sk_solver_free(sk_solver* s);
/* Returns SK_OK and sets *done (boolean) when a termination test fired. */
int sk_solver_step(sk_solver* s, int* done);
int sk_solver_finish(sk_solver* s, sk_summary* summary);
/* Device seconds of kernel `name` accumulated since create, and its launch
 * count (HIP events around the launches when profiling is on).  on: 0 off,
 * 1 every named launch (diagnostic: the event packets slow the small kernels
 * of the panel chain), 2 only the dominant kernel "gemm_syrk". */
int sk_solver_set_kernel_timing(sk_solver* s, int on);
double sk_solver_kernel_seconds(const sk_solver* s, const char* name, int* launches);
/* Algorithmic flop count of the dense Cholesky's trailing updates per linear
 * solve (what roofline.achieved is computed from). */
double sk_solver_syrk_flops_per_solve(const sk_solver* s);
/* Bytes of the C tiles those launches read and write per linear solve (each 128 x 128 tile once in, once out per
 * launch): the algorithmic memory traffic of the trailing updates, next to which bench.py reports the measured one.
 * 0 for solvers that do not report it. */
double sk_solver_syrk_c_bytes_per_solve(const sk_solver* s);
/* SK_DISTRIBUTION_SHARDED or _REPLICATED as decided at sk_solver_create; with AUTO, *allreduce_seconds is the
 * measured all-reduce of the reduced system and *saved_seconds the estimated per-iteration work sharding removes
 * (either pointer may be NULL). */
int sk_solver_distribution(const sk_solver* s, double* allreduce_seconds, double* saved_seconds);
/* Named figures of the solver's plan, for benchmarks and reports (no reference counterpart: Ceres prints the like in
 * Summary::FullReport).  Returns SK_OK and sets *value, or SK_ERR_INVALID_ARGUMENT for a name this solver does not
 * report.  DENSE_SCHUR:
 *   "envelope_fill"         fraction of the lower-triangular 128-blocks of the reduced camera system inside the block
 *                           envelope that is factored (1 with sk_options_set_cholesky_envelope(o, 0))
 *   "camera_order"          0 first appearance, 1 memory order of the camera blocks, 2 reverse Cuthill-McKee
 *   "cholesky_flops_full"   n^3 / 3, n = 9 * cameras: SURVEY.md section 8(d)'s figure for phase C
 *   "cholesky_flops_plan"   flops of the factorisation as planned (potrf + TRSM + updates of the blocks inside the envelope)
 *   "cholesky_columns_resident"  block columns factored under the resident panel chain
 *   "allreduce_bytes"       bytes of the reduced system that travel in the per-iteration all-reduce of the sharded mode (the
 *                           lower block triangle inside the envelope), "allreduce_bytes_full_triangle" beside it
 *   "dissected"             1 when the camera sequence is dissected (sk_options_set_cholesky_dissection), with
 *   "dissection_head_cameras" / "dissection_separator_cameras" / "dissection_tail_cameras" and the model's
 *   "dissection_model_us_plain" / "dissection_model_us" (microseconds of factorisation it predicted either way)
 *   "chain_steps"           serial steps of the factorisation (block columns; two leaf fronts in lock-step count once)
 * every solver:
 *   "phase_seconds_<i>"     seconds accumulated so far in phase i (0 Jacobians, 1 Schur assembly, 2 Cholesky, 3 back-substitution,
 *                           4 candidate cost, 5 all-reduce): sk_summary_phase_seconds, readable between steps
 * DENSE_SCHUR and the dense Jacobian path, each counting since the solver was created:
 *   "linear_solves"         factorisations (of the reduced system; of the normal equations, or QRs) enqueued
 *   "dogleg_reused_steps"   DOGLEG: iterations whose step was re-interpolated from the vectors of an earlier one
 *   "dogleg_mu"             DOGLEG: the current regularisation of the Gauss-Newton solve
 *   "dogleg_w_r" "dogleg_m_r" "dogleg_w_w" "dogleg_w_m" "dogleg_m_m" "dogleg_g_g" "dogleg_g_p" "dogleg_p_p" "dogleg_a" "dogleg_b"
 *                           DOGLEG: the scalars of the last linear solve (w = J s, m = J g over the observations; g-hat and
 *                           the Gauss-Newton step p in the diagonal-scaled space) and the coefficients of the last step a s + b g
 *   "bounded_coordinates"   coordinates with a finite bound (sk_problem_set_parameter_lower_bound / _upper_bound)
 *   "active_bounds"         coordinates of the current x that sit exactly on a bound
 *   "line_search_evaluations" candidate costs evaluated by the line search under bounds, since the solver was created
 * CGNR:
 *   "cg_iterations" CG iterations since the solver was created, "cg_iterations_last" of the last linear solve,
 *   "cg_status_last" how it ended (0 the stopping test, 1 the iteration limit, 2 breakdown, 3 zero right-hand side; -1 before
 *   the first), "cg_batches" reads of the done flag, "jacobian_nonzeros" stored entries of the block-sparse Jacobian,
 *   "schur_elimination" (0 or 1), "eliminated_blocks", "reduced_columns" (all columns without the elimination),
 *   "schur_diagonal_pairs": sk_options_set_schur_elimination
 *   "inner_iteration_steps" LM iterations whose candidate was refined, "inner_iteration_rounds" lock-step rounds since the solver
 *   was created, "inner_iterations_enabled" (1 while the refinement is on), "inner_iteration_seconds" wall time spent refining,
 *   "inner_iteration_groups": sk_options_set_use_inner_iterations
 * dense rows (DENSE_NORMAL_CHOLESKY over one parameter block):
 *   "jtj_flops_algorithmic" m n (n + 1): SURVEY.md section 8(d)'s figure for J^T J (sk_solver_syrk_flops_per_solve counts
 *                           the padded 128 x 128 tiles the launch computes) */
int sk_solver_stat(const sk_solver* s, const char* name, double* value);
/* (no reference counterpart) use_inner_iterations: per parameter block the Levenberg-Marquardt iterations of its solve in the last
 * refinement and how it ended (1 gradient tolerance, 2 parameter tolerance, 3 function tolerance, 4 iteration limit, 5 consecutive
 * invalid steps, 6 minimum radius); -1 for a block that is not refined, and before the first refinement.  Either output may be NULL. */
int sk_solver_inner_iteration_blocks(sk_solver* s, int* iterations, int* status);

/* ---- multi-GPU sharding (host logic, no device needed) -----------------------
 * How sk_solve splits a bundle-adjustment-shaped problem over `world` ranks
 * (SURVEY.md §8e): cameras are the distinct blocks in parameter slot 0, points
 * those in slot 1, both numbered in first-appearance order.  Rank r owns the
 * points [cuts[r], cuts[r+1]) and every observation of them; the runs have
 * (nearly) equal sum of squared track lengths.  `cuts` has world+1 entries.
 * point_of_block[i] (optional, one entry per residual block) receives the point
 * number of residual block i.  Returns SK_ERR_UNSUPPORTED when the problem is
 * not bundle-adjustment shaped. */
int sk_problem_point_partition(const sk_problem* p, int world, int* cuts, int* num_cameras,
                               int* num_points, int* point_of_block);
/* The plan of the SEGMENTED distribution for this problem, from host data alone (no device needed; what every rank derives
 * for itself at set-up): the camera sequence cut into *num_segments segments (at most max_segments; 1 = not cut) with a
 * separator between neighbours.  camera_part_of_block[b] (may be NULL): the segment of residual block b's camera, or -k for a
 * camera of separator k (1 <= k < segments); point_owner_of_block[b] (may be NULL): the rank that owns block b's point.
 * forced != 0: as SK_DISTRIBUTION_SEGMENTED cuts (as many segments as the sequence allows); 0: as AUTO (the chain model's
 * choice).  No point is seen from two segments; a point's blocks all have one owner. */
int sk_problem_segment_plan(const sk_problem* p, int max_segments, int forced, int* num_segments, int* camera_part_of_block,
                            int* point_owner_of_block);
/* The order of the cameras inside the reduced system, and the border of loop-closure cameras (sk_options_set_cholesky_border),
 * as one process derives them at set-up — from host data alone, no device needed.  *num_border_cameras: cameras ordered into
 * the trailing border (0: none); camera_position_of_block[b] (may be NULL): position of residual block b's camera in the
 * reduced system (border cameras: the last *num_border_cameras positions); gap: the jump in a point's camera list that
 * separated visits; model_us / model_us_plain: the chain model's microseconds per factorisation with the order chosen /
 * with the best unbordered order; envelope_fill: 128-blocks inside the envelope over the lower block triangle. */
int sk_problem_border_plan(const sk_problem* p, int mode, int* num_border_cameras, int* camera_position_of_block, int* gap,
                           double* model_us, double* model_us_plain, double* envelope_fill);
/* The retained points (sk_options_set_retained_points) as one process chooses them at set-up — host data alone.  *num_retained:
 * how many (0: none); retained_of_block[b] (may be NULL): 1 when residual block b's point is retained; model_us /
 * model_us_without: the chain model's microseconds per factorisation with them / with every point eliminated (the loop-closure
 * border of `border_mode` in both). */
int sk_problem_retained_plan(const sk_problem* p, int mode, int max_points, int border_mode, int* num_retained, int* retained_of_block,
                             double* model_us, double* model_us_without);

/* ---- inputs of BASELINE.json config 5 (utility) ----------------------------------
 * y_out[i] = tanh(a_i . x_star) for the generated rows a_i of SK_FUNCTOR_SYNTH_TANH_ROW
 * (rows 0 .. m-1 of `seed`, n parameters), computed on the GPU: the planted targets of the
 * synthetic dense problem at sizes where a host loop over m * n generated coefficients is too slow. */
int sk_synth_dense_targets(double seed, int m, int n, const double* x_star, double* y_out);

/* ---- dense SPD solve (utility; the factorisation sk_solve uses) --------------
 * Solves A x = b on the GPU for a symmetric positive definite A (n x n,
 * row-major HOST memory, only the lower triangle is read) with the blocked
 * fp64-MFMA Cholesky.  Optional outputs: L (n x n row-major, lower, upper part
 * zero).  `group` is the SYRK depth in 128-column blocks (0 = default).
 * Returns SK_ERR_EVALUATION_FAILED when A is not positive definite. */
int sk_cholesky_solve(int n, const double* A, const double* b, double* x, double* L, int group);
/* The same with what sk_solve adds for a block-banded reduced camera system.  `last` (optional): the block envelope,
 * one entry per 128-block column of the padded matrix (ceil((n + 1) / 128) of them): last[c] >= c is the last block
 * row in which block column c of the FACTOR can be non-zero (non-decreasing; the final block row, which carries the
 * right-hand side, is always active) — blocks outside are neither read nor written, so A must be zero there.
 * automatic_plan != 0: the grouping is the library's (DENSE_SCHUR's default: resident panel chain where the serial
 * chain decides, launch-by-launch groups where the trailing SYRK does) and `group` <= 0 means 1; otherwise the
 * explicit `group`, launch by launch.  Known-answer tests of the plans sk_solve runs at full size. */
int sk_cholesky_solve_ex(int n, const double* A, const double* b, double* x, double* L, int group, const int* last,
                         int automatic_plan);
/* ... and with a BORDER (sk_options_set_cholesky_border): rows from border_begin_row on are the border — they may couple
 * with any column before them — and the rows before it a block-banded matrix.  The bordered block envelope is derived
 * from A's own non-zero 128-blocks: per block column the run of the band, and the border's block rows from the first
 * block column that reaches them (a border row, once reached, stays active, and so does every border row behind it). */
int sk_cholesky_solve_bordered(int n, const double* A, const double* b, double* x, double* L, int group,
                               int border_begin_row, int automatic_plan);

/* The same system solved by two-way dissection (what DENSE_SCHUR does with the reduced camera system of a camera
 * sequence when that pays — DESIGN.md section 4): rows [0, head) are eliminated front to back, rows [tail_begin, n) back
 * to front, side by side, each leaving its Schur complement on the separator [head, tail_begin), which is factored
 * last.  A(tail, head) must be zero (SK_ERR_INVALID_ARGUMENT otherwise).  The block envelopes of the three fronts are
 * derived from the non-zeros of A.  Known-answer tests of the dissected factorisation against a plain one. */
int sk_cholesky_solve_dissected(int n, const double* A, const double* b, double* x, int head, int tail_begin, int group,
                                int automatic_plan);

/* ... and by multi-way dissection: num_segments >= 2 runs of rows separated by num_segments - 1 separators
 * (cuts[2 (k - 1)], cuts[2 (k - 1) + 1]) = [begin, end) of separator k, ascending; rows behind a separator must not couple
 * with rows before it).  Every segment leaves its Schur complement on the separators next to it — a segment between two
 * separators as a partial factorisation whose border rows of the LEFT separator are active in every column (the spike) —
 * and the separators' block-tridiagonal system is factored last.  This is the arithmetic of the segmented distribution
 * over several GPUs (SK_DISTRIBUTION_SEGMENTED) run on one device: a known-answer test of it. */
int sk_cholesky_solve_segments(int n, const double* A, const double* b, double* x, int num_segments, const int* cuts, int group,
                               int automatic_plan);

#ifdef __cplusplus
}
#endif
#endif /* SKERES_AMD_H */
