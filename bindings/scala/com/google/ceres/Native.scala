package com.google.ceres

// The classes the reference gets from SWIG (ceres.i -> com.google.ceres.*), written by hand over SkeresNative so that
// EX/*.scala and CORE/*.scala keep their imports (`import com.google.ceres._`).  Only what the reference's sources use.
// Not compiled in this repository's image (no scalac); see bindings/README.md.

/** SWIGTYPE_p_double: a native `double*`. */
final class DoublePointer(val address: Long) extends AnyVal { def isNull: Boolean = address == 0L }
/** SWIGTYPE_p_p_double: a native `double**`. */
final class DoublePointerPointer(val address: Long) extends AnyVal { def isNull: Boolean = address == 0L }

/** carrays.i's DoubleArray (ceres.i:95-96): owns `n` native doubles unless made by `frompointer`. */
class DoubleArray private (val address: Long, owned: Boolean) {
  def this(n: Int) = this(SkeresNative.skArrayNew(n), true)
  def getitem(i: Int): Double = SkeresNative.skArrayGetitem(address, i)
  def setitem(i: Int, v: Double): Unit = SkeresNative.skArraySetitem(address, i, v)
  def cast: DoublePointer = new DoublePointer(address)
  override def finalize(): Unit = if (owned) SkeresNative.skArrayFree(address)
}
object DoubleArray { def frompointer(p: DoublePointer): DoubleArray = new DoubleArray(p.address, false) }

/** ceres.i:99-107 */
object DoubleArraySlice { def get(buffer: DoublePointer, start: Int): DoublePointer = new DoublePointer(SkeresNative.skArraySlice(buffer.address, start)) }

/** ceres.i:113-125 */
object DoubleMatrix {
  def isNull(m: DoublePointerPointer): Boolean = m.address == 0L || SkeresNative.skMatrixIsNull(m.address)
  def row(m: DoublePointerPointer, i: Int): DoublePointer = new DoublePointer(SkeresNative.skMatrixRow(m.address, i))
  def toPointerPointer(v: StdVectorDoublePointer): DoublePointerPointer = v.data
}

/** std::vector<double*> (ceres.i:82) */
class StdVectorDoublePointer {
  val handle: Long = SkeresNative.skPtrvecNew()
  /** std::vector<double*>(n): n null pointers (CORE/RichDoubleMatrix.scala:74) */
  def this(n: Int) = { this(); var i = 0; while (i < n) { SkeresNative.skPtrvecAdd(handle, 0L); i += 1 } }
  def add(p: DoublePointer): Unit = SkeresNative.skPtrvecAdd(handle, p.address)
  def set(i: Int, p: DoublePointer): Unit = SkeresNative.skPtrvecSet(handle, i, p.address)
  def get(i: Int): DoublePointer = new DoublePointer(SkeresNative.skPtrvecGet(handle, i))
  def size: Int = SkeresNative.skPtrvecSize(handle)
  /** the vector's storage as a `double**` (DoubleMatrix.toPointerPointer, ceres.i:121-123): valid while the vector lives and is not resized */
  def data: DoublePointerPointer = new DoublePointerPointer(SkeresNative.skPtrvecToPointerPointer(handle))
  override def finalize(): Unit = SkeresNative.skPtrvecFree(handle)
}

/** std::vector<int> (ceres.i:79): what CostFunction's block sizes are to the JVM — `size` is a long and elements are read with
  * `get`, as SWIG's proxy has them (CORE/CostFunctionToFunctor.scala:24-25, CORE/SizedCostFunction.scala:13). */
class StdVectorInt {
  private val values = scala.collection.mutable.ArrayBuffer.empty[Int]
  def add(x: Int): Unit = values += x
  def get(i: Int): Int = values(i)
  def set(i: Int, x: Int): Unit = values(i) = x
  def size: Long = values.length.toLong
  def isEmpty: Boolean = values.isEmpty
  def clear(): Unit = values.clear()
  def toArray: Array[Int] = values.toArray
}

object Ownership extends Enumeration { val DO_NOT_TAKE_OWNERSHIP, TAKE_OWNERSHIP = Value }
object LinearSolverType extends Enumeration { val DENSE_NORMAL_CHOLESKY = Value(0); val DENSE_QR = Value(1); val DENSE_SCHUR = Value(3) }
object MinimizerType extends Enumeration { val LINE_SEARCH = Value(0); val TRUST_REGION = Value(1) }
/** ceres::TrustRegionStrategyType / ceres::DoglegType (ceres/types.h through ceres.i:137). */
object TrustRegionStrategyType extends Enumeration { val LEVENBERG_MARQUARDT = Value(0); val DOGLEG = Value(1) }
object DoglegType extends Enumeration { val TRADITIONAL_DOGLEG = Value(0); val SUBSPACE_DOGLEG = Value(1) }
/** ceres::NumericDiffMethodType (ceres/types.h through ceres.i:137).  A class with members, as SWIG's Java enums are: the reference
  * uses the name as a TYPE (CORE/NumericDiffCostFunction.scala:69, CORE/CostFunctor.scala:62) and imports its members
  * (`import NumericDiffMethodType._`, CORE/NumericDiffCostFunction.scala:80). */
sealed abstract class NumericDiffMethodType(val swigValue: Int)
object NumericDiffMethodType {
  case object CENTRAL extends NumericDiffMethodType(0)
  case object FORWARD extends NumericDiffMethodType(1)
  case object RIDDERS extends NumericDiffMethodType(2)
}
/** ceres::NumericDiffOptions (ceres/numeric_diff_options.h through ceres.i:39,143) with the defaults of Ceres 1.x; plain JVM state —
  * numerically differentiated functors are evaluated on the JVM (CORE/NumericDiffCostFunction.scala:75-162) and reach the solver
  * through the director path. */
class NumericDiffOptions {
  private var relativeStepSize = 1e-6
  private var riddersRelativeInitialStepSize = 1e-2
  private var maxNumRiddersExtrapolations = 10
  private var riddersEpsilon = 1e-12
  private var riddersStepShrinkFactor = 2.0
  def getRelativeStepSize: Double = relativeStepSize
  def setRelativeStepSize(v: Double): Unit = relativeStepSize = v
  def getRiddersRelativeInitialStepSize: Double = riddersRelativeInitialStepSize
  def setRiddersRelativeInitialStepSize(v: Double): Unit = riddersRelativeInitialStepSize = v
  def getMaxNumRiddersExtrapolations: Int = maxNumRiddersExtrapolations
  def setMaxNumRiddersExtrapolations(v: Int): Unit = maxNumRiddersExtrapolations = v
  def getRiddersEpsilon: Double = riddersEpsilon
  def setRiddersEpsilon(v: Double): Unit = riddersEpsilon = v
  def getRiddersStepShrinkFactor: Double = riddersStepShrinkFactor
  def setRiddersStepShrinkFactor(v: Double): Unit = riddersStepShrinkFactor = v
}
object TerminationType extends Enumeration { val CONVERGENCE = Value(0); val NO_CONVERGENCE = Value(1); val FAILURE = Value(2) }

/** ceres::LossFunction as an opaque handle; the JVM proxy owns it (`%newobject`, ceres.i:160-167). */
class LossFunction(val handle: Long) { override def finalize(): Unit = SkeresNative.skLossFree(handle) }
/** ceres.i:168-184 */
object PredefinedLossFunctions {
  def trivialLoss: LossFunction = new LossFunction(SkeresNative.skLossTrivial())
  def huberLoss(a: Double) = new LossFunction(SkeresNative.skLossHuber(a))
  def softLOneLoss(a: Double) = new LossFunction(SkeresNative.skLossSoftLOne(a))
  def cauchyLoss(a: Double) = new LossFunction(SkeresNative.skLossCauchy(a))
  def tukeyLoss(a: Double) = new LossFunction(SkeresNative.skLossTukey(a))
  def tolerantLoss(a: Double, b: Double) = new LossFunction(SkeresNative.skLossTolerant(a, b))
  def composedLoss(f: LossFunction, g: LossFunction) = new LossFunction(SkeresNative.skLossComposed(f.handle, g.handle))
  def scaledLoss(rho: LossFunction, a: Double) = new LossFunction(SkeresNative.skLossScaled(rho.handle, a))
}

class LocalParameterization(val handle: Long) { override def finalize(): Unit = SkeresNative.skLocalParameterizationFree(handle) }
/** ceres.i:192-210 */
object PredefinedLocalParameterizations {
  def identity(size: Int) = new LocalParameterization(SkeresNative.skLocalParameterizationIdentity(size))
  def subset(size: Int, constantParameters: Array[Int]) = new LocalParameterization(SkeresNative.skLocalParameterizationSubset(size, constantParameters))
  def quaternion = new LocalParameterization(SkeresNative.skLocalParameterizationQuaternion())
  def homogeneousVector(size: Int) = new LocalParameterization(SkeresNative.skLocalParameterizationHomogeneousVector(size))
}

/** ceres::CostFunction.  The reference's is a SWIG director (ceres.i:48); here the subclass decides how it reaches native
  * code (SizedCostFunction.nativeHandle): a device functor id, a recorded body, or the director trampoline. */
abstract class CostFunction {
  protected var numResidualsValue = 0
  protected val blockSizes = new StdVectorInt
  def setNumResiduals(n: Int): Unit = numResidualsValue = n
  def numResiduals(): Int = numResidualsValue
  def mutableParameterBlockSizes(): StdVectorInt = blockSizes
  def parameterBlockSizes(): StdVectorInt = blockSizes
  /** CostFunction::Evaluate: `jacobians` may be null, and so may any of its rows. */
  def evaluate(parameters: DoublePointerPointer, residuals: DoublePointer, jacobians: DoublePointerPointer): Boolean
  /** what the native director calls (jvm_evaluate in skeres_amd_jni.c) */
  final def evaluateNative(parameters: Long, residuals: Long, jacobians: Long): Boolean =
    evaluate(new DoublePointerPointer(parameters), new DoublePointer(residuals), new DoublePointerPointer(jacobians))
  /** native sk_cost_function* (created on first use) */
  def nativeHandle: Long
}

/** ceres::Problem, renamed as in ceres.i:73 */
class CeresProblem(options: CeresProblem.Options) {
  val handle: Long = SkeresNative.skProblemNew()
  def addResidualBlock(cost: CostFunction, loss: LossFunction, x: StdVectorDoublePointer): Long =
    SkeresNative.skProblemAddResidualBlock(handle, cost.nativeHandle, if (loss == null) 0L else loss.handle, x.handle)
  def addParameterBlock(values: DoublePointer, size: Int): Unit = SkeresNative.skProblemAddParameterBlock(handle, values.address, size, 0L)
  def addParameterBlock(values: DoublePointer, size: Int, p: LocalParameterization): Unit = SkeresNative.skProblemAddParameterBlock(handle, values.address, size, p.handle)
  def setParameterization(values: DoublePointer, p: LocalParameterization): Unit = SkeresNative.skProblemSetParameterization(handle, values.address, p.handle)
  def setParameterBlockConstant(values: DoublePointer): Unit = SkeresNative.skProblemSetParameterBlockConstant(handle, values.address)
  def setParameterBlockVariable(values: DoublePointer): Unit = SkeresNative.skProblemSetParameterBlockVariable(handle, values.address)
  // ceres::Problem::SetParameterLowerBound / SetParameterUpperBound and their getters (ceres/problem.h via ceres.i:150)
  def setParameterLowerBound(values: DoublePointer, index: Int, bound: Double): Unit = SkeresNative.skProblemSetParameterLowerBound(handle, values.address, index, bound)
  def setParameterUpperBound(values: DoublePointer, index: Int, bound: Double): Unit = SkeresNative.skProblemSetParameterUpperBound(handle, values.address, index, bound)
  def getParameterLowerBound(values: DoublePointer, index: Int): Double = SkeresNative.skProblemGetParameterLowerBound(handle, values.address, index)
  def getParameterUpperBound(values: DoublePointer, index: Int): Double = SkeresNative.skProblemGetParameterUpperBound(handle, values.address, index)
  def numResidualBlocks: Int = SkeresNative.skProblemNumResidualBlocks(handle)
  def numParameterBlocks: Int = SkeresNative.skProblemNumParameterBlocks(handle)
  /** (no reference counterpart) the block's index in the problem's own order (first mention), -1 when it is none of its blocks */
  def parameterBlockIndex(block: DoublePointer): Int = SkeresNative.skProblemParameterBlockIndex(handle, block.address)
  def numParameters: Int = SkeresNative.skProblemNumParameters(handle)
  def numResiduals: Int = SkeresNative.skProblemNumResiduals(handle)
  /** ceres::Problem::Evaluate (ceres/problem.h via ceres.i) at the current contents of the parameter memory, on the device: the cost,
    * and — where the caller passes an array of the right length, or asks for it — residuals, gradient and the Jacobian as a CRSMatrix.
    * Rows follow evalOptions' residual blocks (all, in the order added), columns its parameter blocks (all, in the order first seen),
    * each with its tangent size; a constant block keeps its columns and stores nothing. */
  def evaluate(evalOptions: CeresProblem.EvaluateOptions, wantResiduals: Boolean, wantGradient: Boolean, wantJacobian: Boolean): CeresProblem.Evaluation = {
    val o = if (evalOptions == null) 0L else evalOptions.handle
    val sizes = new Array[Long](3)
    SkeresNative.skProblemEvaluateSizes(handle, o, sizes)
    val cost = new Array[Double](1)
    val residuals = if (wantResiduals) new Array[Double](sizes(0).toInt) else null
    val gradient = if (wantGradient) new Array[Double](sizes(1).toInt) else null
    val jacobian = if (wantJacobian) evaluateStructure(evalOptions) else null
    SkeresNative.skProblemEvaluate(handle, o, cost, residuals, gradient, if (jacobian == null) null else jacobian.values)
    new CeresProblem.Evaluation(cost(0), residuals, gradient, jacobian)
  }
  def evaluate(evalOptions: CeresProblem.EvaluateOptions): CeresProblem.Evaluation = evaluate(evalOptions, true, true, true)
  /** The CRSMatrix evaluate would fill, its values zero: host logic, no device needed. */
  def evaluateStructure(evalOptions: CeresProblem.EvaluateOptions): CRSMatrix = {
    val o = if (evalOptions == null) 0L else evalOptions.handle
    val sizes = new Array[Long](3)
    SkeresNative.skProblemEvaluateSizes(handle, o, sizes)
    val m = new CRSMatrix(sizes(0).toInt, sizes(1).toInt, new Array[Int](sizes(0).toInt + 1), new Array[Int](sizes(2).toInt), new Array[Double](sizes(2).toInt))
    SkeresNative.skProblemEvaluateStructure(handle, o, m.rows, m.cols)
    m
  }
  override def finalize(): Unit = SkeresNative.skProblemFree(handle)
}
/** ceres::CRSMatrix (ceres/crs_matrix.h via ceres.i): row r holds cols / values [rows(r), rows(r + 1)). */
class CRSMatrix(val numRows: Int, val numCols: Int, val rows: Array[Int], val cols: Array[Int], val values: Array[Double])
object CeresProblem {
  /** ceres::Problem::EvaluateOptions; empty lists mean all; num_threads has no counterpart. */
  class EvaluateOptions {
    val handle: Long = SkeresNative.skEvaluateOptionsNew()
    def setApplyLossFunction(on: Boolean): Unit = SkeresNative.skEvaluateOptionsSetApplyLossFunction(handle, if (on) 1 else 0)
    def setResidualBlocks(ids: Array[Int]): Unit = SkeresNative.skEvaluateOptionsSetResidualBlocks(handle, ids)
    def setParameterBlocks(blocks: Seq[DoublePointer]): Unit = SkeresNative.skEvaluateOptionsSetParameterBlocks(handle, blocks.map(_.address).toArray)
    def setDevice(device: Int): Unit = SkeresNative.skEvaluateOptionsSetDevice(handle, device)
    override def finalize(): Unit = SkeresNative.skEvaluateOptionsFree(handle)
  }
  class Evaluation(val cost: Double, val residuals: Array[Double], val gradient: Array[Double], val jacobian: CRSMatrix)
  /** The native problem never owns cost or loss functions (sk_problem_new): the setters exist for source compatibility. */
  class Options { def setCostFunctionOwnership(o: Ownership.Value): Unit = (); def setLossFunctionOwnership(o: Ownership.Value): Unit = () }
}

/** ceres::Covariance (ceres/covariance.h via ceres.i:29,141): blocks of (J^T J)^-1 at the current contents of the parameter memory, by the
  * Cholesky factorisation of the scaled normal matrix on the device.  compute answers false where the Jacobian is rank deficient (there
  * is no pseudo-inverse); the getters return row-major arrays, size(a) x size(b) or, in the tangent space, tangent(a) x tangent(b). */
class Covariance(options: Covariance.Options) {
  val handle: Long = SkeresNative.skCovarianceNew(if (options == null) 0L else options.handle)
  /** Covariance::Compute(covariance_blocks, problem) */
  def compute(covarianceBlocks: Seq[(DoublePointer, DoublePointer)], problem: CeresProblem): Boolean =
    SkeresNative.skCovarianceCompute(handle, problem.handle, covarianceBlocks.map(_._1.address).toArray, covarianceBlocks.map(_._2.address).toArray) == 0
  /** Covariance::Compute(parameter_blocks, problem): every pair among the blocks */
  def computeBlocks(parameterBlocks: Seq[DoublePointer], problem: CeresProblem): Boolean =
    SkeresNative.skCovarianceComputeBlocks(handle, problem.handle, parameterBlocks.map(_.address).toArray) == 0
  private def sizeOf(block: DoublePointer, tangent: Boolean): Int = {
    val sizes = new Array[Int](2)
    SkeresNative.skCovarianceBlockSizes(handle, block.address, sizes)
    if (tangent) sizes(1) else sizes(0)
  }
  private def block(a: DoublePointer, b: DoublePointer, tangent: Boolean): Array[Double] = {
    val out = new Array[Double](math.max(1, sizeOf(a, tangent) * sizeOf(b, tangent)))
    SkeresNative.skCovarianceGetBlock(handle, a.address, b.address, if (tangent) 1 else 0, out)
    out
  }
  private def matrix(blocks: Seq[DoublePointer], tangent: Boolean): Array[Double] = {
    val dim = blocks.map(sizeOf(_, tangent)).sum
    val out = new Array[Double](math.max(1, dim * dim))
    SkeresNative.skCovarianceGetMatrix(handle, blocks.map(_.address).toArray, if (tangent) 1 else 0, out)
    out
  }
  def getCovarianceBlock(a: DoublePointer, b: DoublePointer): Array[Double] = block(a, b, false)
  def getCovarianceBlockInTangentSpace(a: DoublePointer, b: DoublePointer): Array[Double] = block(a, b, true)
  def getCovarianceMatrix(blocks: Seq[DoublePointer]): Array[Double] = matrix(blocks, false)
  def getCovarianceMatrixInTangentSpace(blocks: Seq[DoublePointer]): Array[Double] = matrix(blocks, true)
  /** "columns", "selected_columns", "normal_matrix_pairs", "reciprocal_pivot_ratio", "schur_elimination", "eliminated_blocks", "reduced_columns",
    * "schur_terms", "phase_seconds_0".."phase_seconds_4" of the last compute */
  def stat(name: String): Double = SkeresNative.skCovarianceStat(handle, name)
  override def finalize(): Unit = SkeresNative.skCovarianceFree(handle)
}
object Covariance {
  /** ceres::Covariance::Options; algorithm_type, null_space_rank and num_threads have no counterpart. */
  class Options {
    val handle: Long = SkeresNative.skCovarianceOptionsNew()
    def setApplyLossFunction(on: Boolean): Unit = SkeresNative.skCovarianceOptionsSetApplyLossFunction(handle, if (on) 1 else 0)
    def setMinReciprocalConditionNumber(v: Double): Unit = SkeresNative.skCovarianceOptionsSetMinReciprocalConditionNumber(handle, v)
    def setDevice(device: Int): Unit = SkeresNative.skCovarianceOptionsSetDevice(handle, device)
    /** (no reference counterpart; default off) eliminate an independent set of blocks — in bundle adjustment the points — in front of
      * the dense factorisation: the route for problems of more than 32 768 columns (include/skeres_amd.h). */
    def setSchurElimination(on: Boolean): Unit = SkeresNative.skCovarianceOptionsSetSchurElimination(handle, if (on) 1 else 0)
    override def finalize(): Unit = SkeresNative.skCovarianceOptionsFree(handle)
  }
  /** The eliminated set of setSchurElimination for this problem, from host data alone (sk_covariance_elimination_plan). */
  class EliminationPlan(val eliminatedOfBlock: Array[Int], val numEliminated: Int, val reducedColumns: Int, val schurTerms: Long)
  def eliminationPlan(problem: CeresProblem): EliminationPlan = {
    val ofBlock = new Array[Int](math.max(1, problem.numParameterBlocks))
    val counts = new Array[Int](2)
    val terms = new Array[Long](1)
    SkeresNative.skCovarianceEliminationPlan(problem.handle, ofBlock, counts, terms)
    new EliminationPlan(ofBlock.take(problem.numParameterBlocks), counts(0), counts(1), terms(0))
  }
}

object Solver {
  class Options {
    val handle: Long = SkeresNative.skOptionsNew()
    def setLinearSolverType(t: LinearSolverType.Value): Unit = SkeresNative.skOptionsSetLinearSolverType(handle, t.id)
    def setMinimizerType(t: MinimizerType.Value): Unit = SkeresNative.skOptionsSetMinimizerType(handle, t.id)
    def setTrustRegionStrategyType(t: TrustRegionStrategyType.Value): Unit = SkeresNative.skOptionsSetTrustRegionStrategyType(handle, t.id)
    def setDoglegType(t: DoglegType.Value): Unit = SkeresNative.skOptionsSetDoglegType(handle, t.id)
    def trustRegionStrategyType: TrustRegionStrategyType.Value = TrustRegionStrategyType(SkeresNative.skOptionsGetTrustRegionStrategyType(handle))
    def doglegType: DoglegType.Value = DoglegType(SkeresNative.skOptionsGetDoglegType(handle))
    def setMaxNumIterations(n: Int): Unit = SkeresNative.skOptionsSetMaxNumIterations(handle, n)
    def setMinimizerProgressToStdout(on: Boolean): Unit = SkeresNative.skOptionsSetMinimizerProgressToStdout(handle, if (on) 1 else 0)
    def setFunctionTolerance(v: Double): Unit = SkeresNative.skOptionsSetFunctionTolerance(handle, v)
    def setGradientTolerance(v: Double): Unit = SkeresNative.skOptionsSetGradientTolerance(handle, v)
    def setParameterTolerance(v: Double): Unit = SkeresNative.skOptionsSetParameterTolerance(handle, v)
    def setInitialTrustRegionRadius(v: Double): Unit = SkeresNative.skOptionsSetInitialTrustRegionRadius(handle, v)
    def setMaxTrustRegionRadius(v: Double): Unit = SkeresNative.skOptionsSetMaxTrustRegionRadius(handle, v)
    def setMinTrustRegionRadius(v: Double): Unit = SkeresNative.skOptionsSetMinTrustRegionRadius(handle, v)
    def setMinRelativeDecrease(v: Double): Unit = SkeresNative.skOptionsSetMinRelativeDecrease(handle, v)
    def setMinLmDiagonal(v: Double): Unit = SkeresNative.skOptionsSetMinLmDiagonal(handle, v)
    def setMaxLmDiagonal(v: Double): Unit = SkeresNative.skOptionsSetMaxLmDiagonal(handle, v)
    def setJacobiScaling(on: Boolean): Unit = SkeresNative.skOptionsSetJacobiScaling(handle, if (on) 1 else 0)
    def setMaxNumConsecutiveInvalidSteps(n: Int): Unit = SkeresNative.skOptionsSetMaxNumConsecutiveInvalidSteps(handle, n)
    // MI355X additions (no counterpart in ceres::Solver::Options)
    def setDevice(hipDevice: Int): Unit = SkeresNative.skOptionsSetDevice(handle, hipDevice)
    def setDistributionMode(mode: Int): Unit = SkeresNative.skOptionsSetDistributionMode(handle, mode)
    /** CGNR: conjugate gradients on the implicit Schur complement of an independent set of parameter blocks (default off) */
    def setSchurElimination(on: Boolean): Unit = SkeresNative.skOptionsSetSchurElimination(handle, if (on) 1 else 0)
    /** CGNR: after every trust-region step each parameter block of an independent set is minimised on its own, set after set
      * (Solver::Options::use_inner_iterations; default off; every other linear solver type refuses it when the solver is created) */
    def setUseInnerIterations(on: Boolean): Unit = SkeresNative.skOptionsSetUseInnerIterations(handle, if (on) 1 else 0)
    def getUseInnerIterations: Boolean = SkeresNative.skOptionsGetUseInnerIterations(handle) != 0
    def setInnerIterationTolerance(v: Double): Unit = SkeresNative.skOptionsSetInnerIterationTolerance(handle, v)
    def getInnerIterationTolerance: Double = SkeresNative.skOptionsGetInnerIterationTolerance(handle)
    /** group id -> the native pointers of its parameter blocks (ceres::ParameterBlockOrdering's group_to_elements); empty: automatic */
    def setInnerIterationOrdering(groupToElements: Map[Int, Seq[Long]]): Unit = {
      val pairs = groupToElements.toSeq.sortBy(_._1).flatMap { case (g, blocks) => blocks.map(b => (b, g)) }
      SkeresNative.skOptionsSetInnerIterationOrdering(handle, pairs.map(_._1).toArray, pairs.map(_._2).toArray)
    }
    /** this JVM is rank `rank` of `world`, one per GPU; the collective is the library's own RCCL all-reduce */
    def setDistributedRccl(rank: Int, world: Int, uniqueId: Array[Byte]): Unit = {
      rccl = SkeresNative.skAllreduceRcclInit(rank, world, uniqueId)
      SkeresNative.skOptionsSetDistributedRccl(handle, rank, world, rccl)
    }
    private var rccl = 0L
    override def finalize(): Unit = { SkeresNative.skOptionsFree(handle); if (rccl != 0L) SkeresNative.skAllreduceRcclFree(rccl) }
  }
  class Summary {
    val handle: Long = SkeresNative.skSummaryNew()
    def initialCost: Double = SkeresNative.skSummaryInitialCost(handle)
    def finalCost: Double = SkeresNative.skSummaryFinalCost(handle)
    def numSuccessfulSteps: Int = SkeresNative.skSummaryNumSuccessfulSteps(handle)
    def numUnsuccessfulSteps: Int = SkeresNative.skSummaryNumUnsuccessfulSteps(handle)
    def terminationType: TerminationType.Value = TerminationType(SkeresNative.skSummaryTerminationType(handle))
    // (they differ when DENSE_SCHUR met a problem without the 2 / (9, 3) block structure: its alternate, DENSE_QR, was used — as Ceres does)
    def linearSolverTypeUsed: LinearSolverType.Value = LinearSolverType(SkeresNative.skSummaryLinearSolverTypeUsed(handle))
    def linearSolverTypeGiven: LinearSolverType.Value = LinearSolverType(SkeresNative.skSummaryLinearSolverTypeGiven(handle))
    def message: String = SkeresNative.skSummaryMessage(handle)
    def briefReport(): String = SkeresNative.skSummaryBriefReport(handle)
    def fullReport(): String = SkeresNative.skSummaryFullReport(handle)
    override def finalize(): Unit = SkeresNative.skSummaryFree(handle)
  }
}

/** the module class of ceres.i: free functions */
object ceres {
  def initGoogleLogging(name: String): Unit = SkeresNative.skInitLogging(name)
  def solve(options: Solver.Options, problem: CeresProblem, summary: Solver.Summary): Unit =
    SkeresNative.skSolve(options.handle, problem.handle, summary.handle)
}
