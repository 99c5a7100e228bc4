// miFoam.C -- see miFoam.H.  Host code only; every number is produced by the HIP engine behind
// the C ABI (include/mi_ldu.h).  Compiled with hipcc only because device memory is managed here.
#include "miFoam.H"

#include <array>

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <ctime>
#include <limits>

namespace Foam
{

std::ostream& Info = std::cout;

void FatalErrorIn(const std::string& where, const std::string& msg)
{
    // the reference prints "--> FOAM FATAL ERROR" and aborts (error.C); a library throws instead
    throw error("--> FOAM FATAL ERROR:\n" + msg + "\n\n    From function " + where);
}

void miCheck(int rc, const char* where)
{
    if (rc != MI_OK) FatalErrorIn(where, std::string("MI355X engine error ") + std::to_string(rc) + ": " + mi_last_error());
}

#define FOAM_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) FatalErrorIn(#expr, hipGetErrorString(e_)); } while (0)

// one engine context per process = per MPI rank = per GPU (argList.C:775-811 `-device N`)
struct miEngine
{
    mi_ctx_t ctx;
    miEngine() : ctx(nullptr)
    {
        const char* d = std::getenv("MI_DEVICE");
        miCheck(mi_ctx_create(d ? std::atoi(d) : 0, nullptr, &ctx), "miEngine::miEngine()");
    }
    ~miEngine() { mi_ctx_destroy(ctx); }
    static miEngine& New() { static miEngine e; return e; }
};

void* miDeviceAlloc(std::size_t bytes) { miEngine::New(); void* p = nullptr; FOAM_HIP(hipMalloc(&p, bytes)); return p; }
void miDeviceFree(void* p) { (void)hipFree(p); }
void miCopyH2D(void* d, const void* s, std::size_t n) { FOAM_HIP(hipMemcpy(d, s, n, hipMemcpyHostToDevice)); }
void miCopyD2H(void* d, const void* s, std::size_t n) { mi_ctx_synchronize(miEngine::New().ctx); FOAM_HIP(hipMemcpy(d, s, n, hipMemcpyDeviceToHost)); }
void miCopyD2D(void* d, const void* s, std::size_t n) { mi_ctx_synchronize(miEngine::New().ctx); FOAM_HIP(hipMemcpy(d, s, n, hipMemcpyDeviceToDevice)); }
void miDeviceZero(void* p, std::size_t n) { FOAM_HIP(hipMemset(p, 0, n)); }

// ---- solverPerformance ------------------------------------------------------------------------------
const scalar solverPerformance::great_ = 1e20;
const scalar solverPerformance::small_ = 1e-20;
const scalar solverPerformance::vsmall_ = 1e-300;

bool solverPerformance::checkConvergence(scalar tol, scalar relTol)
{
    converged_ = (finalResidual_ < tol) || (relTol > small_ && finalResidual_ < relTol * initialResidual_);
    return converged_;
}
bool solverPerformance::checkSingularity(scalar residual) { singular_ = residual < vsmall_; return singular_; }
void solverPerformance::print(std::ostream& os) const
{
    os << solverName_ << ":  Solving for " << fieldName_;
    if (singular_) os << ":  solution singularity" << std::endl;
    else os << ", Initial residual = " << initialResidual_ << ", Final residual = " << finalResidual_
            << ", No Iterations " << noIterations_ << std::endl;
}

// ---- lduAddressing --------------------------------------------------------------------------------------
lduAddressing::lduAddressing(label nCells, const labelList& lower, const labelList& upper, const std::vector<labelList>& patchAddr)
: size_(nCells), lower_(lower), upper_(upper), patchAddr_(patchAddr), addr_(nullptr), gamg_(nullptr), gamgCoarsest_(-1)
{
    if (lower_.size() != upper_.size()) FatalErrorIn("lduAddressing::lduAddressing", "lowerAddr and upperAddr differ in size");
    for (const labelList& fc : patchAddr_) { lduInterface i; i.faceCells = fc; interfaces_.push_back(i); }
}
lduAddressing::lduAddressing(label nCells, const labelList& lower, const labelList& upper, const std::vector<lduInterface>& interfaces)
: size_(nCells), lower_(lower), upper_(upper), interfaces_(interfaces), addr_(nullptr), gamg_(nullptr), gamgCoarsest_(-1)
{
    if (lower_.size() != upper_.size()) FatalErrorIn("lduAddressing::lduAddressing", "lowerAddr and upperAddr differ in size");
    for (const lduInterface& i : interfaces_) patchAddr_.push_back(i.faceCells);
    for (std::size_t p = 0; p < interfaces_.size(); ++p) {
        const lduInterface& i = interfaces_[p];
        if (i.type == "cyclic" && (i.neighbPatchID < 0 || i.neighbPatchID >= (label)interfaces_.size() ||
                                    interfaces_[i.neighbPatchID].faceCells.size() != i.faceCells.size()))
            FatalErrorIn("lduAddressing::lduAddressing", "cyclic patch without a matching neighbour patch");
        if (i.type == "cyclicAMI" && (i.neighbPatchID < 0 || i.neighbPatchID >= (label)interfaces_.size() || i.amiStart.size() != i.faceCells.size() + 1))
            FatalErrorIn("lduAddressing::lduAddressing", "cyclicAMI patch without a neighbour patch / AMI addressing");
        if (i.type != "cyclic" && i.type != "processor" && i.type != "coupled" && i.type != "cyclicAMI") FatalErrorIn("lduAddressing::lduAddressing", "Unknown interface type " + i.type);
    }
}
lduAddressing::~lduAddressing() { if (gamg_) mi_gamg_destroy(gamg_); if (addr_) mi_addr_destroy(addr_); }
mi_addr_t lduAddressing::handle() const
{
    if (!addr_) {
        std::vector<label> sizes; std::vector<const label*> ptrs, nbrs;
        for (std::size_t p = 0; p < patchAddr_.size(); ++p) {
            sizes.push_back((label)patchAddr_[p].size()); ptrs.push_back(patchAddr_[p].data());
            const bool plainCyclic = interfaces_[p].type == "cyclic" && !interfaces_[p].transforms;
            nbrs.push_back(plainCyclic ? patchAddr_[(std::size_t)interfaces_[p].neighbPatchID].data() : nullptr);
        }
        miCheck(mi_addr_create_coupled(miEngine::New().ctx, size_, (label)lower_.size(), lower_.data(), upper_.data(), (label)sizes.size(),
                                       sizes.data(), ptrs.data(), nbrs.data(), &addr_), "lduAddressing::handle()");
        for (std::size_t p = 0; p < interfaces_.size(); ++p) {
            const lduInterface& i = interfaces_[p];
            if (i.type == "cyclicAMI") {
                miCheck(mi_addr_set_ami_patch(addr_, (label)p, i.neighbPatchID, i.amiStart.data(), i.amiAddress.data(), i.amiWeights.data(),
                                              i.amiLowWeight.empty() ? nullptr : i.amiLowWeight.data()), "cyclicAMILduInterface");
                if (!i.amiMagSf.empty()) miCheck(mi_addr_set_ami_face_areas(addr_, (label)p, i.amiMagSf.data()), "cyclicAMILduInterface");
            } else if (i.type == "cyclic" && i.transforms)
                miCheck(mi_addr_set_ami_patch(addr_, (label)p, i.neighbPatchID, nullptr, nullptr, nullptr, nullptr), "cyclicLduInterface (transformed)");
        }
    }
    return addr_;
}
mi_gamg_t lduAddressing::dummyAgglomeration(label nLevels) const
{   // agglomerator dummy (dummyAgglomeration.C:45-90): cached like the pair agglomerations, keyed by -nLevels
    if (gamg_ && gamgCoarsest_ != -nLevels) { mi_gamg_destroy(gamg_); gamg_ = nullptr; }
    if (!gamg_) { miCheck(mi_gamg_create_dummy(handle(), nLevels, &gamg_), "dummyAgglomeration::dummyAgglomeration"); gamgCoarsest_ = -nLevels; gamgMerge_ = 1; }
    return gamg_;
}
mi_gamg_t lduAddressing::agglomeration(const scalarField& w, label nCoarsest, label mergeLevels) const
{
    if (gamg_ && (gamgCoarsest_ != nCoarsest || gamgMerge_ != mergeLevels)) { mi_gamg_destroy(gamg_); gamg_ = nullptr; }
    if (!gamg_) {
        if ((label)w.size() != (label)lower_.size()) FatalErrorIn("lduAddressing::agglomeration", "face weights do not match the number of faces");
        if (hasProcessorPatches() || Pstream::parRun()) {
            if (!Pstream::parRun()) FatalErrorIn("GAMGAgglomeration::New", "processor patches outside a parallel run (Pstream::init)");
            std::vector<label> pr, pn;
            for (const lduInterface& i : interfaces_) { pr.push_back(i.neighbProcNo); pn.push_back(i.neighbPatchID); }
            miCheck(mi_gamg_create_coupled(handle(), w.data(), nCoarsest, mergeLevels, 1, Pstream::reduceComm(), Pstream::haloComm(),
                                           pr.data(), pn.data(), &gamg_), "GAMGAgglomeration::New");
        } else
        miCheck(mi_gamg_create(handle(), w.data(), nCoarsest, mergeLevels, 1, &gamg_), "GAMGAgglomeration::New");
        gamgCoarsest_ = nCoarsest; gamgMerge_ = mergeLevels;
    }
    return gamg_;
}

// ---- lduMatrix ----------------------------------------------------------------------------------------------
lduMatrix::lduMatrix(const lduAddressing& a)
: lduAddr_(a), diag_(a.size()), upper_((label)a.lowerAddrHost().size()), mat_(nullptr), dirty_(true) {}
lduMatrix::~lduMatrix() { if (mat_) mi_matrix_destroy(mat_); }
scalargpuField& lduMatrix::lower()
{
    if (!lowerPtr_) lowerPtr_.reset(new scalargpuField(upper_));
    dirty_ = true;
    return *lowerPtr_;
}
void lduMatrix::sync(const FieldFieldScalar* bou, const FieldFieldScalar* inte, const lduInterfaceFieldPtrsList* ifs) const
{
    if (!mat_) miCheck(mi_matrix_create(lduAddr_.handle(), &mat_), "lduMatrix::sync");
    if (dirty_) { // the reference's lowerSortPtr_ invalidation (lduMatrix.C:235,266)
        miCheck(mi_matrix_set_coeffs(mat_, diag_.data(), upper_.data(), lowerPtr_ ? lowerPtr_->data() : nullptr), "lduMatrix::sync");
        dirty_ = false;
    }
    const label nP = lduAddr_.nPatches();
    if (nP == 0 && Pstream::parRun() && !attached_) {
        miCheck(mi_matrix_attach_comm(mat_, Pstream::reduceComm(), Pstream::haloComm(), nullptr, nullptr,
                                      Pstream::returnReduceSum(lduAddr_.size())), "lduMatrix::sync");
        attached_ = true;
    }
    if (nP == 0) return;
    if (!bou || (label)bou->size() != nP || !ifs || (label)ifs->size() != nP)
        FatalErrorIn("lduMatrix::sync", "interface coefficient lists do not match the coupled patches of the addressing");
    const bool callerExt = !lduAddr_.engineCoupled();
    scalargpuField ext(callerExt ? mi_addr_n_ext(lduAddr_.handle()) : 0);
    label off = 0;
    for (label p = 0; p < nP; ++p) {
        const label n = (label)lduAddr_.patchAddr(p).size();
        miCheck(mi_matrix_set_interface_coeffs(mat_, p, (*bou)[p].data(), inte && (label)inte->size() == nP ? (*inte)[p].data() : nullptr), "lduMatrix::sync");
        if ((*ifs)[p]->doTransform() || transformSet_) { // transformCoupleField(pnf, cmpt) of this solve's component
            miCheck(mi_matrix_set_patch_transform(mat_, p, (*ifs)[p]->transformFactor(cmpt_)), "lduMatrix::sync");
            transformSet_ = true;
        }
        if (callerExt && n) miCopyD2D(ext.data() + off, (*ifs)[p]->patchNeighbourField.data(), sizeof(scalar) * n);
        off += n;
    }
    if (callerExt) miCheck(mi_matrix_set_ext(mat_, ext.data()), "lduMatrix::sync");
    if (!attached_ && (lduAddr_.hasProcessorPatches() || Pstream::parRun())) {
        // decomposed case: from here on the engine exchanges the processor-patch values and all-reduces the sums itself
        if (!Pstream::parRun()) FatalErrorIn("lduMatrix::sync", "processor patches outside a parallel run (Pstream::init)");
        std::vector<label> pr, pn;
        for (label p = 0; p < nP; ++p) { pr.push_back(lduAddr_.interface(p).neighbProcNo); pn.push_back(lduAddr_.interface(p).neighbPatchID); }
        miCheck(mi_matrix_attach_comm(mat_, Pstream::reduceComm(), Pstream::haloComm(), pr.data(), pn.data(),
                                      Pstream::returnReduceSum(lduAddr_.size())), "lduMatrix::sync");
        attached_ = true;
    }
    mi_ctx_synchronize(miEngine::New().ctx);
}
void lduMatrix::Amul(scalargpuField& Apsi, const scalargpuField& psi, const FieldFieldScalar& b, const lduInterfaceFieldPtrsList& ifs, direction cmpt) const
{
    cmpt_ = cmpt; sync(&b, nullptr, &ifs); miCheck(mi_amul(mat_, psi.data(), Apsi.data()), "lduMatrix::Amul");
}
void lduMatrix::Tmul(scalargpuField& Tpsi, const scalargpuField& psi, const FieldFieldScalar& i, const lduInterfaceFieldPtrsList& ifs, direction cmpt) const
{
    cmpt_ = cmpt;
    // Tmul uses interfaceIntCoeffs (lduMatrixATmul.C:264-342): pass them in both slots so the engine's lower side holds them
    sync(&i, &i, &ifs); miCheck(mi_tmul(mat_, psi.data(), Tpsi.data()), "lduMatrix::Tmul");
    dirty_ = true;
}
void lduMatrix::sumA(scalargpuField& s, const FieldFieldScalar& b, const lduInterfaceFieldPtrsList& ifs) const
{
    sync(&b, nullptr, &ifs); miCheck(mi_sumA(mat_, s.data()), "lduMatrix::sumA");
}
void lduMatrix::patchNeighbourField(FieldFieldScalar& nbr, const scalargpuField& psi, const FieldFieldScalar& b, const lduInterfaceFieldPtrsList& ifs) const
{
    sync(&b, nullptr, &ifs);
    label nExt = 0;
    for (const lduInterfaceField* f : ifs) nExt += (label)f->faceCells.size();
    scalargpuField all(nExt);
    miCheck(mi_matrix_patch_neighbour_field(mat_, psi.data(), all.data()), "coupledFvPatchField::patchNeighbourField");
    const std::vector<scalar> h = all.asHost();
    nbr.clear();
    std::size_t off = 0;
    for (const lduInterfaceField* f : ifs) {
        const std::size_t n = f->faceCells.size();
        nbr.push_back(scalargpuField(scalarField(h.begin() + (std::ptrdiff_t)off, h.begin() + (std::ptrdiff_t)(off + n))));
        off += n;
    }
}
void lduMatrix::residual(scalargpuField& rA, const scalargpuField& psi, const scalargpuField& source, const FieldFieldScalar& b,
                         const lduInterfaceFieldPtrsList& ifs, direction cmpt) const
{
    cmpt_ = cmpt; sync(&b, nullptr, &ifs); miCheck(mi_residual(mat_, psi.data(), source.data(), rA.data()), "lduMatrix::residual");
}
void lduMatrix::negSumDiag() { miCheck(mi_row_face_op(lduAddr_.handle(), 1, lowerPtr_ ? lowerPtr_->data() : nullptr, upper_.data(), diag_.data()), "lduMatrix::negSumDiag"); dirty_ = true; }
void lduMatrix::sumDiag() { miCheck(mi_row_face_op(lduAddr_.handle(), 0, lowerPtr_ ? lowerPtr_->data() : nullptr, upper_.data(), diag_.data()), "lduMatrix::sumDiag"); dirty_ = true; }
void lduMatrix::sumMagOffDiag(scalargpuField& s) const { miCheck(mi_row_face_op(lduAddr_.handle(), 2, lowerPtr_ ? lowerPtr_->data() : nullptr, upper_.data(), s.data()), "lduMatrix::sumMagOffDiag"); }

// ---- preconditioner names (lduMatrixPreconditioner.C:36-65) ---------------------------------------------------
word lduMatrix::preconditioner::getName(const dictionary& d)
{
    word name = d.lookup("preconditioner");
    // DIC / DILU (and friends) are replaced by the approximate inverse in the reference
    // (DICPreconditioner.C:42-58, DILUPreconditioner.C:42-58): the reported name becomes AINV
    if (name == "DIC" || name == "DILU") name = "AINV";
    return name;
}
int lduMatrix::preconditioner::kindFor(const dictionary& d, bool sym)
{
    const word name = d.lookup("preconditioner");
    const bool ok = name == "AINV" || name == "diagonal" || name == "none" || name == (sym ? "DIC" : "DILU");
    if (!ok)
        FatalErrorIn("lduMatrix::preconditioner::New(const solver&, const dictionary&)",
                     word("Unknown ") + (sym ? "symmetric" : "asymmetric") + " matrix preconditioner " + name + "\n\nValid " + (sym ? "symmetric" : "asymmetric")
                     + " matrix preconditioners :\n" + (sym ? "4(AINV DIC diagonal none)" : "4(AINV DILU diagonal none)"));
    return kind(getName(d));
}
int lduMatrix::preconditioner::kind(const word& n)
{
    if (n == "none") return MI_PRECOND_NONE;
    if (n == "diagonal") return MI_PRECOND_DIAGONAL;
    if (n == "AINV") return MI_PRECOND_AINV;
    FatalErrorIn("lduMatrix::preconditioner::New", "Unknown preconditioner " + n + "\n\nValid preconditioners are :\n(AINV DIC DILU diagonal none)");
}

// ---- solver base + factory --------------------------------------------------------------------------------------
std::map<word, lduMatrix::solver::ctor>& lduMatrix::solver::symMatrixConstructorTable() { static std::map<word, ctor> t; return t; }
std::map<word, lduMatrix::solver::ctor>& lduMatrix::solver::asymMatrixConstructorTable() { static std::map<word, ctor> t; return t; }

lduMatrix::solver::solver(const word& fieldName, const lduMatrix& matrix, const FieldFieldScalar& b, const FieldFieldScalar& i,
                          const lduInterfaceFieldPtrsList& ifs, const dictionary& d)
: fieldName_(fieldName), matrix_(matrix), interfaceBouCoeffs_(b), interfaceIntCoeffs_(i), interfaces_(ifs), controlDict_(d)
{
    readControls();
}
void lduMatrix::solver::readControls()
{
    maxIter_ = controlDict_.lookupOrDefault<label>("maxIter", 1000);
    minIter_ = controlDict_.lookupOrDefault<label>("minIter", 0);
    tolerance_ = controlDict_.lookupOrDefault<scalar>("tolerance", 1e-6);
    relTol_ = controlDict_.lookupOrDefault<scalar>("relTol", 0);
}

namespace
{
word tableNames(const std::map<word, lduMatrix::solver::ctor>& t)
{
    word s = "(";
    for (auto& kv : t) s += kv.first + " ";
    if (s.size() > 1) s.pop_back();
    return s + ")";
}
mi_solver_controls controlsOf(scalar tol, scalar relTol, label maxIter, label minIter) { mi_solver_controls c = {tol, relTol, maxIter, minIter}; return c; }
solverPerformance perfOf(const word& solverName, const word& fieldName, const mi_solver_perf& r)
{
    return solverPerformance(solverName, fieldName, r.initialResidual, r.finalResidual, r.nIterations, r.converged != 0, r.singular != 0);
}
// whole-solver calls own the exchange: fine for cyclic / processor interfaces (the engine does it), not for interfaces
// whose neighbour values the caller supplies once (they would go stale inside the iteration)
void requireUncoupled(const lduInterfaceFieldPtrsList& ifs, const char* who)
{
    for (const lduInterfaceField* f : ifs)
        if (f && f->type() == "coupled")
            FatalErrorIn(who, "interfaces with caller-supplied neighbour values cannot be iterated on: use cyclicLduInterfaceField / processorLduInterfaceField");
}
} // namespace

// diagonalSolver (solvers/diagonalSolver/diagonalSolver.C): psi = source/diag
class diagonalSolver : public lduMatrix::solver
{
public:
    using lduMatrix::solver::solver;
    solverPerformance solve(scalargpuField& psi, const scalargpuField& source, const direction) const override
    {
        std::vector<scalar> d = matrix_.diag().asHost(), s = source.asHost();
        for (std::size_t i = 0; i < d.size(); ++i) s[i] /= d[i];
        psi = s;
        return solverPerformance("diagonalSolver", fieldName_, 0, 0, 0, true, false);
    }
};

autoPtr<lduMatrix::solver> lduMatrix::solver::New(const word& fieldName, const lduMatrix& matrix, const FieldFieldScalar& b,
                                                  const FieldFieldScalar& i, const lduInterfaceFieldPtrsList& ifs, const dictionary& d)
{
    const word name = d.lookup("solver");
    if (matrix.diagonal()) return autoPtr<solver>(new diagonalSolver(fieldName, matrix, b, i, ifs, d));
    const bool sym = matrix.symmetric();
    auto& table = sym ? symMatrixConstructorTable() : asymMatrixConstructorTable();
    auto it = table.find(name);
    if (it == table.end())
        FatalErrorIn("lduMatrix::solver::New", "Unknown " + word(sym ? "symmetric" : "asymmetric") + " matrix solver " + name +
                     "\n\nValid " + word(sym ? "symmetric" : "asymmetric") + " matrix solvers are :\n" + tableNames(table));
    return it->second(fieldName, matrix, b, i, ifs, d);
}

// ---- concrete solvers, registered under the reference's run-time names ---------------------------------------------
class PCG : public lduMatrix::solver
{
public:
    using lduMatrix::solver::solver;
    solverPerformance solve(scalargpuField& psi, const scalargpuField& source, const direction cmpt) const override
    {
        requireUncoupled(interfaces_, "PCG::solve");
        const word pre = lduMatrix::preconditioner::getName(controlDict_);
        const mi_solver_controls c = controlsOf(tolerance_, relTol_, maxIter_, minIter_);
        mi_solver_perf r;
        miCheck(mi_pcg_solve(matrix_.handle(interfaceBouCoeffs_, interfaceIntCoeffs_, interfaces_, cmpt), psi.data(), source.data(), &c,
                             lduMatrix::preconditioner::kindFor(controlDict_, matrix_.symmetric()), &r, nullptr, 0), "PCG::solve");
        return perfOf(pre + "PCG", fieldName_, r); // PCG.C:75-80
    }
};
class PBiCG : public lduMatrix::solver
{
public:
    using lduMatrix::solver::solver;
    solverPerformance solve(scalargpuField& psi, const scalargpuField& source, const direction cmpt) const override
    {
        requireUncoupled(interfaces_, "PBiCG::solve");
        const word pre = lduMatrix::preconditioner::getName(controlDict_);
        const mi_solver_controls c = controlsOf(tolerance_, relTol_, maxIter_, minIter_);
        mi_solver_perf r;
        miCheck(mi_pbicg_solve(matrix_.handle(interfaceBouCoeffs_, interfaceIntCoeffs_, interfaces_, cmpt), psi.data(), source.data(), &c,
                               lduMatrix::preconditioner::kindFor(controlDict_, matrix_.symmetric()), &r, nullptr, 0), "PBiCG::solve");
        return perfOf(pre + "PBiCG", fieldName_, r);
    }
};
class PBiCGStab : public lduMatrix::solver
{
public:
    using lduMatrix::solver::solver;
    solverPerformance solve(scalargpuField& psi, const scalargpuField& source, const direction cmpt) const override
    {
        requireUncoupled(interfaces_, "PBiCGStab::solve");
        const word pre = lduMatrix::preconditioner::getName(controlDict_);
        const mi_solver_controls c = controlsOf(tolerance_, relTol_, maxIter_, minIter_);
        mi_solver_perf r;
        // keep the reference's `psi += omega*yA` (PBiCGStab.C:263-270) unless the case asks for the textbook update
        const int quirk = controlDict_.lookupOrDefault<label>("textbookOmegaUpdate", 0) ? 0 : 1;
        miCheck(mi_pbicgstab_solve(matrix_.handle(interfaceBouCoeffs_, interfaceIntCoeffs_, interfaces_, cmpt), psi.data(), source.data(), &c,
                                   lduMatrix::preconditioner::kindFor(controlDict_, matrix_.symmetric()), quirk, &r, nullptr, 0), "PBiCGStab::solve");
        return perfOf(pre + "PBiCGStab", fieldName_, r);
    }
};
class smoothSolver : public lduMatrix::solver
{
public:
    using lduMatrix::solver::solver;
    solverPerformance solve(scalargpuField& psi, const scalargpuField& source, const direction cmpt) const override
    {
        requireUncoupled(interfaces_, "smoothSolver::solve");
        const word sm = controlDict_.lookup("smoother");
        if (sm != "GaussSeidel" && sm != "Jacobi") // GaussSeidelSmoother.C:43-66: GaussSeidel IS Jacobi in the reference
            FatalErrorIn("lduMatrix::smoother::New", "Unknown smoother " + sm + "\n\nValid smoothers are :\n(GaussSeidel Jacobi)");
        const mi_solver_controls c = controlsOf(tolerance_, relTol_, maxIter_, minIter_);
        mi_solver_perf r;
        miCheck(mi_smooth_solve(matrix_.handle(interfaceBouCoeffs_, interfaceIntCoeffs_, interfaces_, cmpt), psi.data(), source.data(), &c,
                                controlDict_.lookupOrDefault<scalar>("omega", 0.9), controlDict_.lookupOrDefault<label>("nSweeps", 1),
                                &r, nullptr, 0), "smoothSolver::solve");
        return perfOf("smoothSolver", fieldName_, r);
    }
};
class GAMGSolver : public lduMatrix::solver
{
public:
    using lduMatrix::solver::solver;
    solverPerformance solve(scalargpuField& psi, const scalargpuField& source, const direction cmpt) const override
    {
        requireUncoupled(interfaces_, "GAMGSolver::solve");
        const word agg = controlDict_.lookupOrDefault<word>("agglomerator", "faceAreaPair");
        const label nCoarsest = controlDict_.lookupOrDefault<label>("nCellsInCoarsestLevel", -1);
        if (nCoarsest < 0) FatalErrorIn("GAMGAgglomeration::GAMGAgglomeration", "keyword nCellsInCoarsestLevel is undefined in dictionary"); // GAMGAgglomeration.C:96-99
        if (agg != "dummy" && !controlDict_.found("mergeLevels")) FatalErrorIn("pairGAMGAgglomeration::pairGAMGAgglomeration", "keyword mergeLevels is undefined in dictionary");
        if (agg == "dummy" && !controlDict_.found("nLevels")) FatalErrorIn("dummyAgglomeration::dummyAgglomeration", "keyword nLevels is undefined in dictionary"); // dummyAgglomeration.C:52
        {   // GAMGSolver.C:75: interpolateCorrection (default false).  The reference's interpolate() overload that every level
            // with a coarser level calls starts with notImplemented() (GAMGSolverInterpolate.C:180), i.e. it aborts: same here.
            const word ic = controlDict_.lookupOrDefault<word>("interpolateCorrection", "false");
            if (ic == "true" || ic == "on" || ic == "yes" || ic == "y" || ic == "t") FatalErrorIn("GAMGSolver::interpolate()", "Not implemented");
        }
        const label mergeLevels = controlDict_.lookupOrDefault<label>("mergeLevels", 1);
        if (mergeLevels < 1) FatalErrorIn("pairGAMGAgglomeration::pairGAMGAgglomeration", "mergeLevels must be positive");
        const word sm = controlDict_.lookupOrDefault<word>("smoother", "GaussSeidel");
        if (sm != "GaussSeidel" && sm != "Jacobi") FatalErrorIn("lduMatrix::smoother::New", "Unknown smoother " + sm);
        scalarField w;
        if (agg == "algebraicPair") { w = matrix_.upper().asHost(); for (scalar& v : w) v = std::fabs(v); } // algebraicPairGAMGAgglomeration.C:47-61
        else if (agg == "faceAreaPair") {
            const word key = "faceAreaPairWeights";  // supplied by the mesh layer (faceAreaPairGAMGAgglomeration.C:54-81)
            if (!faceWeights_) FatalErrorIn("faceAreaPairGAMGAgglomeration", "no face-area weights registered for this mesh (" + key + ")");
            w = *faceWeights_;
        } else if (agg != "dummy") FatalErrorIn("GAMGAgglomeration::New", "Unknown GAMGAgglomeration type " + agg);
        mi_gamg_t g = agg == "dummy" ? matrix_.lduAddr().dummyAgglomeration(controlDict_.lookupOrDefault<label>("nLevels", 1))
                                     : matrix_.lduAddr().agglomeration(w, nCoarsest, mergeLevels);
        mi_gamg_controls c;
        c.tolerance = tolerance_; c.relTol = relTol_; c.maxIter = maxIter_; c.minIter = minIter_;
        c.nPreSweeps = controlDict_.lookupOrDefault<label>("nPreSweeps", 0);
        c.preSweepsLevelMultiplier = controlDict_.lookupOrDefault<label>("preSweepsLevelMultiplier", 1);
        c.maxPreSweeps = controlDict_.lookupOrDefault<label>("maxPreSweeps", 4);
        c.nPostSweeps = controlDict_.lookupOrDefault<label>("nPostSweeps", 2);
        c.postSweepsLevelMultiplier = controlDict_.lookupOrDefault<label>("postSweepsLevelMultiplier", 1);
        c.maxPostSweeps = controlDict_.lookupOrDefault<label>("maxPostSweeps", 4);
        c.nFinestSweeps = controlDict_.lookupOrDefault<label>("nFinestSweeps", 2);
        c.scaleCorrection = controlDict_.found("scaleCorrection") ? controlDict_.lookupOrDefault<label>("scaleCorrection", 1) : -1;
        c.omega = controlDict_.lookupOrDefault<scalar>("omega", 0.9);
        {   // GAMGSolver.C:77,232: directSolveCoarsest (default true in this code base); false = ICCG / BICCG on the coarsest level
            const word ds = controlDict_.lookupOrDefault<word>("directSolveCoarsest", "true");
            c.directSolveCoarsest = (ds == "false" || ds == "off" || ds == "no" || ds == "n" || ds == "f") ? 0 : 1;
            c.reserved = 0;
        }
        mi_solver_perf r;
        miCheck(mi_gamg_solve(g, matrix_.handle(interfaceBouCoeffs_, interfaceIntCoeffs_, interfaces_, cmpt), psi.data(), source.data(), &c, &r, nullptr, 0), "GAMGSolver::solve");
        return perfOf("GAMG", fieldName_, r);
    }
    static const scalarField* faceWeights_;
};
const scalarField* GAMGSolver::faceWeights_ = nullptr;
void setFaceAreaPairWeights(const scalarField* w) { GAMGSolver::faceWeights_ = w; }

// static registration objects, as in PCG.C:36-37 etc.
static lduMatrix::solver::addsymMatrixConstructorToTable<PCG> addPCGSymMatrixConstructorToTable_("PCG");
static lduMatrix::solver::addasymMatrixConstructorToTable<PBiCG> addPBiCGAsymMatrixConstructorToTable_("PBiCG");
static lduMatrix::solver::addasymMatrixConstructorToTable<PBiCGStab> addPBiCGStabAsymMatrixConstructorToTable_("PBiCGStab");
// ICCG / BICCG (solvers/ICCG/ICCG.C:34-35, solvers/BICCG/BICCG.C:34-35): PCG / PBiCG under another run-time name; constructed
// from a dictionary they pass it on unchanged, so the preconditioner is the dictionary's and the printed name is PCG's / PBiCG's
class ICCG : public PCG { public: using PCG::PCG; };
class BICCG : public PBiCG { public: using PBiCG::PBiCG; };
static lduMatrix::solver::addsymMatrixConstructorToTable<ICCG> addICCGSymMatrixConstructorToTable_("ICCG");
static lduMatrix::solver::addasymMatrixConstructorToTable<BICCG> addBICCGSymMatrixConstructorToTable_("BICCG");
static lduMatrix::solver::addsymMatrixConstructorToTable<smoothSolver> addsmoothSolverSymMatrixConstructorToTable_("smoothSolver");
static lduMatrix::solver::addasymMatrixConstructorToTable<smoothSolver> addsmoothSolverAsymMatrixConstructorToTable_("smoothSolver");
static lduMatrix::solver::addsymMatrixConstructorToTable<GAMGSolver> addGAMGSolverMatrixConstructorToTable_("GAMG");
static lduMatrix::solver::addasymMatrixConstructorToTable<GAMGSolver> addGAMGAsymSolverMatrixConstructorToTable_("GAMG");

// ---- fvScalarMatrix -----------------------------------------------------------------------------------------------------
fvScalarMatrix::fvScalarMatrix(const word& psiName, const lduAddressing& a, const std::vector<labelList>& pfc, const std::vector<bool>& coupled)
: lduMatrix(a), psiName_(psiName), source_(a.size()), patchFaceCells_(pfc), patchCoupled_(coupled)
{
    for (const labelList& p : pfc) { internalCoeffs_.emplace_back((label)p.size()); boundaryCoeffs_.emplace_back((label)p.size()); }
    patches_.assign(pfc.size(), nullptr);
}
fvScalarMatrix::~fvScalarMatrix() { for (mi_patch_t p : patches_) if (p) mi_patch_destroy(p); }
static mi_patch_t patchOf(std::vector<mi_patch_t>& cache, std::size_t k, label nCells, const labelList& fc)
{
    if (!cache[k]) miCheck(mi_patch_create(miEngine::New().ctx, nCells, (label)fc.size(), fc.data(), &cache[k]), "fvPatch::faceCells");
    return cache[k];
}
void fvScalarMatrix::addBoundaryDiag(scalargpuField& diag) const
{
    for (std::size_t p = 0; p < patchFaceCells_.size(); ++p)
        miCheck(mi_patch_add(patchOf(patches_, p, lduAddr().size(), patchFaceCells_[p]), internalCoeffs_[p].data(), diag.data(), 0), "fvMatrix::addBoundaryDiag");
}
void fvScalarMatrix::addBoundarySource(scalargpuField& source, const std::vector<const scalargpuField*>& patchNeighbourField) const
{
    for (std::size_t p = 0; p < patchFaceCells_.size(); ++p) {
        if (!patchCoupled_[p])
            miCheck(mi_patch_add(patchOf(patches_, p, lduAddr().size(), patchFaceCells_[p]), boundaryCoeffs_[p].data(), source.data(), 0), "fvMatrix::addBoundarySource");
        else if (p < patchNeighbourField.size() && patchNeighbourField[p])
            miCheck(mi_patch_add_product(patchOf(patches_, p, lduAddr().size(), patchFaceCells_[p]), boundaryCoeffs_[p].data(),
                                         patchNeighbourField[p]->data(), source.data(), 0), "fvMatrix::addBoundarySource");
    }
}
void fvScalarMatrix::relax(scalar alpha, const scalargpuField& psi)
{
    std::vector<mi_patch_t> ph; std::vector<const double*> ic, bc; std::vector<int32_t> cp;
    for (std::size_t p = 0; p < patchFaceCells_.size(); ++p) {
        ph.push_back(patchOf(patches_, p, lduAddr().size(), patchFaceCells_[p]));
        ic.push_back(internalCoeffs_[p].data()); bc.push_back(boundaryCoeffs_[p].data()); cp.push_back(patchCoupled_[p] ? 1 : 0);
    }
    miCheck(mi_relax(lduAddr().handle(), alpha, diag().data(), asymmetric() ? lower().data() : nullptr, upper().data(), source_.data(), psi.data(),
                     (label)ph.size(), ph.data(), ic.data(), bc.data(), cp.data()), "fvMatrix::relax");
}
void fvScalarMatrix::setReference(label celli, scalar value)
{
    miCheck(mi_fvm_set_reference(lduAddr().handle(), celli, value, diag().data(), source_.data()), "fvMatrix::setReference");
}
void fvScalarMatrix::setValues(const labelgpuList& cellLabels, const scalargpuField& values, scalargpuField& psi)
{
    std::vector<mi_patch_t> ph; std::vector<double*> ic, bc;
    for (std::size_t p = 0; p < patchFaceCells_.size(); ++p) {
        ph.push_back(patchOf(patches_, p, lduAddr().size(), patchFaceCells_[p]));
        ic.push_back(internalCoeffs_[p].data()); bc.push_back(boundaryCoeffs_[p].data());
    }
    const bool wasSym = !asymmetric();
    const scalargpuField upperIn(upper());            // (the non-const lower() below copies upper, as the reference's does)
    scalargpuField& lo = lower();
    miCheck(mi_fvm_set_values(lduAddr().handle(), cellLabels.size(), cellLabels.data(), values.data(), 0, psi.data(), diag().data(), source_.data(),
                              upperIn.data(), wasSym ? nullptr : lo.data(), upper().data(), lo.data(), (label)ph.size(), ph.data(), ic.data(), bc.data()),
            "fvMatrix::setValues");
}
solverPerformance fvScalarMatrix::solve(scalargpuField& psi, const dictionary& solverControls)
{
    // fvScalarMatrix.C:142-192: saveDiag; addBoundaryDiag; totalSource = source + boundary; solver::New()->solve; restore
    scalargpuField saveDiag(diag());
    addBoundaryDiag(diag());
    scalargpuField totalSource(source_);
    addBoundarySource(totalSource);
    FieldFieldScalar noCoeffs; lduInterfaceFieldPtrsList noInterfaces;
    solverPerformance perf = lduMatrix::solver::New(psiName_, *this, noCoeffs, noCoeffs, noInterfaces, solverControls)->solve(psi, totalSource);
    perf.print(Info);
    diag() = saveDiag;
    return perf;
}

solverPerformance max(const solverPerformance& a, const solverPerformance& b)
{
    solverPerformance r(a.solverName(), a.fieldName(), std::max(a.initialResidual(), b.initialResidual()),
                        std::max(a.finalResidual(), b.finalResidual()), std::max(a.nIterations(), b.nIterations()),
                        a.converged() && b.converged(), a.singular() || b.singular());
    return r;
}

// ---- fvVectorMatrix ---------------------------------------------------------------------------------------------------
fvVectorMatrix::fvVectorMatrix(const word& psiName, const lduAddressing& a, const std::vector<labelList>& pfc, const std::vector<bool>& coupled)
: lduMatrix(a), psiName_(psiName), source_(a.size()), patchFaceCells_(pfc), patchCoupled_(coupled)
{
    for (const labelList& p : pfc) { internalCoeffs_.emplace_back((label)p.size()); boundaryCoeffs_.emplace_back((label)p.size()); }
    patches_.assign(pfc.size(), nullptr);
}
fvVectorMatrix::~fvVectorMatrix() { for (mi_patch_t p : patches_) if (p) mi_patch_destroy(p); }
void fvVectorMatrix::addBoundaryDiag(scalargpuField& diag, direction cmpt) const
{
    for (std::size_t p = 0; p < patchFaceCells_.size(); ++p)
        miCheck(mi_patch_add(patchOf(patches_, p, lduAddr().size(), patchFaceCells_[p]), internalCoeffs_[p].component(cmpt).data(), diag.data(), 0), "fvMatrix::addBoundaryDiag");
}
void fvVectorMatrix::addBoundarySource(vectorgpuField& source) const
{
    for (std::size_t p = 0; p < patchFaceCells_.size(); ++p)
        if (!patchCoupled_[p])
            for (direction d = 0; d < 3; ++d)
                miCheck(mi_patch_add(patchOf(patches_, p, lduAddr().size(), patchFaceCells_[p]), boundaryCoeffs_[p].component(d).data(), source.component(d).data(), 0), "fvMatrix::addBoundarySource");
}
solverPerformance fvVectorMatrix::solve(vectorgpuField& psi, const dictionary& solverControls)
{
    static const char* componentNames[3] = {"x", "y", "z"};
    solverPerformance solverPerfVec("fvMatrix<Type>::solveSegregated", psiName_);
    scalargpuField saveDiag(diag());
    vectorgpuField source(lduAddr().size());
    for (direction d = 0; d < 3; ++d) source.component(d) = source_.component(d);
    addBoundarySource(source);
    FieldFieldScalar noCoeffs; lduInterfaceFieldPtrsList noInterfaces;
    // MI355X form of the component loop: PBiCG on the three components as ONE solve (mi_pbicg_solve_multi) -- every pass over
    // upper / lower serves all components, each component keeps its own diagonal (addBoundaryDiag(diag, cmpt)), scalars,
    // convergence test and solverPerformance line; same numbers as the loop below (`segregatedLoop yes;` selects that)
    if (asymmetric() && solverControls.lookup("solver") == "PBiCG" && solverControls.lookupOrDefault<word>("segregatedLoop", "no") != "yes") {
        std::vector<scalargpuField> dc;
        dc.reserve(3);
        const double* dptr[3]; double* pptr[3]; const double* sptr[3];
        for (direction cmpt = 0; cmpt < 3; ++cmpt) {
            dc.emplace_back(saveDiag);
            addBoundaryDiag(dc.back(), cmpt);
        }
        for (direction cmpt = 0; cmpt < 3; ++cmpt) { dptr[cmpt] = dc[cmpt].data(); pptr[cmpt] = psi.component(cmpt).data(); sptr[cmpt] = source.component(cmpt).data(); }
        const mi_solver_controls c = controlsOf(solverControls.lookupOrDefault<scalar>("tolerance", 1e-6), solverControls.lookupOrDefault<scalar>("relTol", 0),
                                                solverControls.lookupOrDefault<label>("maxIter", 1000), solverControls.lookupOrDefault<label>("minIter", 0));
        mi_solver_perf r[3];
        miCheck(mi_pbicg_solve_multi(handle(noCoeffs, noCoeffs, noInterfaces, 0), 3, dptr, pptr, sptr, &c,
                                     lduMatrix::preconditioner::kindFor(solverControls, false), r, nullptr, 0), "fvMatrix<Type>::solveSegregated");
        const word pre = lduMatrix::preconditioner::getName(solverControls);
        for (direction cmpt = 0; cmpt < 3; ++cmpt) {
            solverPerformance solverPerf = perfOf(pre + "PBiCG", psiName_ + componentNames[cmpt], r[cmpt]);
            solverPerf.print(Info);
            solverPerformance m = max(solverPerfVec, solverPerf);
            solverPerfVec = solverPerformance(solverPerf.solverName(), psiName_, m.initialResidual(), m.finalResidual(), m.nIterations(), m.converged(), m.singular());
        }
        return solverPerfVec;
    }
    for (direction cmpt = 0; cmpt < 3; ++cmpt) {
        addBoundaryDiag(diag(), cmpt);
        solverPerformance solverPerf = lduMatrix::solver::New(psiName_ + componentNames[cmpt], *this, noCoeffs, noCoeffs, noInterfaces, solverControls)
                                           ->solve(psi.component(cmpt), source.component(cmpt), cmpt);
        solverPerf.print(Info);
        solverPerformance m = max(solverPerfVec, solverPerf);
        solverPerfVec = solverPerformance(solverPerf.solverName(), psiName_, m.initialResidual(), m.finalResidual(), m.nIterations(),
                                          m.converged(), m.singular()); // (the reference's vector perf starts unconverged, so it stays so)
        diag() = saveDiag;
    }
    return solverPerfVec;
}

void fvVectorMatrix::A(scalargpuField& Aphi, const scalargpuField& V) const
{
    mi_ctx_t ctx = miEngine::New().ctx;
    Aphi = diag();
    for (std::size_t p = 0; p < patchFaceCells_.size(); ++p) {
        const label np = (label)patchFaceCells_[p].size();
        if (np == 0) continue;
        scalargpuField av(np), three(std::vector<scalar>((std::size_t)np, 3.0));       // cmptAv(v) = (v.x() + v.y() + v.z())/3
        miCheck(mi_vec_axpby(ctx, np, 1.0, internalCoeffs_[p].component(0).data(), 1.0, internalCoeffs_[p].component(1).data(), av.data()), "cmptAv");
        miCheck(mi_vec_axpby(ctx, np, 1.0, av.data(), 1.0, internalCoeffs_[p].component(2).data(), av.data()), "cmptAv");
        miCheck(mi_vec_div(ctx, np, av.data(), three.data(), av.data()), "cmptAv");
        miCheck(mi_patch_add(patchOf(patches_, p, lduAddr().size(), patchFaceCells_[p]), av.data(), Aphi.data(), 0), "fvMatrix::addCmptAvBoundaryDiag");
    }
    miCheck(mi_vec_div(ctx, Aphi.size(), Aphi.data(), V.data(), Aphi.data()), "fvMatrix::A");
}
void fvVectorMatrix::H(vectorgpuField& Hphi, const vectorgpuField& psi, const scalargpuField& V) const
{
    static const FieldFieldScalar none; static const lduInterfaceFieldPtrsList noIfs;
    mi_ctx_t ctx = miEngine::New().ctx;
    for (direction d = 0; d < 3; ++d) {
        miCheck(mi_H(handle(none, none, noIfs), psi.component(d).data(), Hphi.component(d).data()), "lduMatrix::H");
        miCheck(mi_vec_axpby(ctx, Hphi.size(), 1.0, Hphi.component(d).data(), 1.0, source_.component(d).data(), Hphi.component(d).data()), "fvMatrix::H");
    }
    addBoundarySource(Hphi);
    for (direction d = 0; d < 3; ++d) miCheck(mi_vec_div(ctx, Hphi.size(), Hphi.component(d).data(), V.data(), Hphi.component(d).data()), "fvMatrix::H");
}
namespace {
mi_div_correction divCorrection(const linearUpwindCorrection& corr, std::size_t nRhs)
{
    if (!corr.Cf || !corr.C || corr.grad.size() != nRhs) FatalErrorIn("linearUpwind::correction", "one gradient per component of the field is needed");
    mi_div_correction k{};
    k.scale = corr.scale;
    for (int d = 0; d < 3; ++d) { k.cf_dev[d] = corr.Cf->component(d).data(); k.c_dev[d] = corr.C->component(d).data(); }
    for (std::size_t r = 0; r < nRhs; ++r) {
        if (!corr.grad[r]) FatalErrorIn("linearUpwind::correction", "null gradient");
        for (int d = 0; d < 3; ++d) k.grad_dev[3 * r + d] = corr.grad[r]->component(d).data();
    }
    return k;
}
// the time form of one fvm::assemble: rDeltaT is Euler's and backward's 1/deltaT or CrankNicolson's rDtCoef; fields: backward's old-old fields /
// CrankNicolson's ddt0 fields, one per right-hand side
struct ddtForm
{
    enum { Euler, backward, CrankNicolson } kind;
    scalar rDeltaT;
    const backwardDdtCoeffs* bd;
    scalar ocCoeff;
    const scalargpuField* const* fields;
};
// the worker of every fvm::assemble: the terms, the time form's part and the optional correction, then the one matching C entry (corr / su nullptr: none)
void assembleTerms(const char* where, lduMatrix& M, scalargpuField* const* sources, const ddtForm& f, scalar rho, const scalargpuField& V,
                   const scalargpuField* const* psiOld, int nRhs, const scalargpuField* faceFlux, const scalargpuField* weights, const scalargpuField* deltaCoeffs,
                   const scalargpuField* gammaMagSf, const linearUpwindCorrection* corr, const scalargpuField* su)
{
    mi_fvm_terms t{};
    t.ddt = 1; t.r_delta_t = f.rDeltaT; t.rho_value = rho; t.vol_dev = V.data();
    t.div_flux_dev = faceFlux ? faceFlux->data() : nullptr; t.div_weights_dev = weights ? weights->data() : nullptr;
    t.lap_delta_coeffs_dev = deltaCoeffs ? deltaCoeffs->data() : nullptr; t.lap_gamma_magsf_dev = gammaMagSf ? gammaMagSf->data() : nullptr;
    const double *po[3], *tf[3]; double* so[3];
    for (int r = 0; r < nRhs; ++r) { po[r] = psiOld[r]->data(); so[r] = sources[r]->data(); if (f.kind != ddtForm::Euler) tf[r] = f.fields[r]->data(); }
    t.n_rhs = nRhs; t.psi_old_dev = po;
    const double* sd[1] = {su ? su->data() : nullptr}; const double sg[1] = {1.0};
    if (su) { t.n_su = 1; t.su_dev = sd; t.su_sign = sg; }
    mi_div_correction k{};
    if (corr) k = divCorrection(*corr, (std::size_t)nRhs);
    const mi_div_correction* kp = corr ? &k : nullptr;
    const mi_addr_t a = M.lduAddr().handle();
    double *lower = faceFlux ? M.lower().data() : nullptr, *upper = M.upper().data(), *diag = M.diag().data();
    if (f.kind == ddtForm::backward) {
        mi_ddt_backward b{};
        b.coefft = f.bd->coefft; b.coefft0 = f.bd->coefft0; b.coefft00 = f.bd->coefft00; b.psi_old_old_dev = tf;
        miCheck(mi_fvm_assemble_backward(a, &t, &b, kp, lower, upper, diag, so, nullptr), where);
    } else if (f.kind == ddtForm::CrankNicolson) {
        mi_ddt_cn_terms c{};
        c.oc = f.ocCoeff; c.ddt0_dev = tf;
        miCheck(mi_fvm_assemble_cn(a, &t, &c, kp, lower, upper, diag, so, nullptr), where);
    } else if (corr)
        miCheck(mi_fvm_assemble_corrected(a, &t, kp, lower, upper, diag, so, nullptr), where);
    else
        miCheck(mi_fvm_assemble(a, &t, lower, upper, diag, so, nullptr), where);
}
ddtForm EulerForm(scalar rDeltaT) { return {ddtForm::Euler, rDeltaT, nullptr, 0, nullptr}; }
}
void fvm::assemble(fvVectorMatrix& M, scalar rDeltaT, scalar rho, const scalargpuField& V, const vectorgpuField& psiOld, const scalargpuField* faceFlux,
                   const scalargpuField* weights, const scalargpuField* deltaCoeffs, const scalargpuField* gammaMagSf)
{
    assembleTerms("fvm::assemble", M, cmpts(M.source()), EulerForm(rDeltaT), rho, V, cmpts(psiOld), 3, faceFlux, weights, deltaCoeffs, gammaMagSf, nullptr, nullptr);
}
void fvm::laplacian(fvScalarMatrix& M, const scalargpuField& deltaCoeffs, const scalargpuField& gammaMagSf)
{
    miCheck(mi_fvm_laplacian(M.lduAddr().handle(), deltaCoeffs.data(), gammaMagSf.data(), M.upper().data(), M.diag().data()), "fvm::laplacian");
}
void fvm::div(fvScalarMatrix& M, const scalargpuField& weights, const scalargpuField& faceFlux)
{
    scalargpuField& lower = M.lower();
    miCheck(mi_fvm_div(M.lduAddr().handle(), weights.data(), faceFlux.data(), lower.data(), M.upper().data(), M.diag().data()), "fvm::div");
}

// ---- fvMatrix operators and the scheme front-end ------------------------------------------------------------------
void fvScalarMatrix::axpyFrom(const fvScalarMatrix& B, scalar b)
{
    if (&B.lduAddr() != &lduAddr()) FatalErrorIn("fvMatrix::operator+=", "incompatible matrices: different addressing");
    mi_ctx_t ctx = miEngine::New().ctx;
    auto ax = [&](scalargpuField& x, const scalargpuField& y) {
        if (x.size() != y.size()) FatalErrorIn("fvMatrix::operator+=", "incompatible fields");
        if (x.size()) miCheck(mi_vec_axpby(ctx, x.size(), 1.0, x.data(), b, y.data(), x.data()), "fvMatrix::operator+=");
    };
    if (B.asymmetric() && symmetric()) lower();                 // promote: lower becomes a copy of upper first
    if (asymmetric()) ax(lower(), B.lower());                    // B.lower() aliases B.upper() when B is symmetric
    ax(upper(), B.upper()); ax(diag(), B.diag()); ax(source_, B.source_);
    for (std::size_t p = 0; p < internalCoeffs_.size(); ++p) { ax(internalCoeffs_[p], B.internalCoeffs_[p]); ax(boundaryCoeffs_[p], B.boundaryCoeffs_[p]); }
}
void fvScalarMatrix::A(scalargpuField& Aphi, const scalargpuField& V) const
{
    Aphi = diag();
    addBoundaryDiag(Aphi);
    miCheck(mi_vec_div(miEngine::New().ctx, Aphi.size(), Aphi.data(), V.data(), Aphi.data()), "fvMatrix::A");
}
void fvScalarMatrix::H(scalargpuField& Hphi, const scalargpuField& psi, const scalargpuField& V,
                       const std::vector<const scalargpuField*>& patchNeighbourField) const
{
    static const FieldFieldScalar none; static const lduInterfaceFieldPtrsList noIfs;
    miCheck(mi_H(handle(none, none, noIfs), psi.data(), Hphi.data()), "lduMatrix::H");
    mi_ctx_t ctx = miEngine::New().ctx;
    miCheck(mi_vec_axpby(ctx, Hphi.size(), 1.0, Hphi.data(), 1.0, source_.data(), Hphi.data()), "fvMatrix::H");
    addBoundarySource(Hphi, patchNeighbourField);
    miCheck(mi_vec_div(ctx, Hphi.size(), Hphi.data(), V.data(), Hphi.data()), "fvMatrix::H");
}
void fvScalarMatrix::flux(scalargpuField& internalFlux, FieldFieldScalar& boundaryFlux, const scalargpuField& psi,
                          const std::vector<const scalargpuField*>& patchNeighbourField) const
{
    static const FieldFieldScalar none; static const lduInterfaceFieldPtrsList noIfs;
    miCheck(mi_faceH(handle(none, none, noIfs), psi.data(), internalFlux.data()), "lduMatrix::faceH");
    if (boundaryFlux.size() != patchFaceCells_.size()) boundaryFlux.resize(patchFaceCells_.size());
    for (std::size_t p = 0; p < patchFaceCells_.size(); ++p) {
        if (boundaryFlux[p].size() != (label)patchFaceCells_[p].size()) boundaryFlux[p] = scalargpuField((label)patchFaceCells_[p].size());
        const scalargpuField* nbr = (patchCoupled_[p] && p < patchNeighbourField.size()) ? patchNeighbourField[p] : nullptr;
        if (patchCoupled_[p] && !nbr) throw error("fvMatrix::flux: coupled patch without patchNeighbourField");
        miCheck(mi_patch_flux(patchOf(patches_, p, lduAddr().size(), patchFaceCells_[p]), internalCoeffs_[p].data(), boundaryCoeffs_[p].data(),
                              psi.data(), nbr ? nbr->data() : nullptr, boundaryFlux[p].data()), "fvMatrix::flux");
    }
}
void fvScalarMatrix::gaussGradOf(vectorgpuField& g, const scalargpuField& vf, const std::vector<const scalargpuField*>& patchValues, const vectorgpuField& Sf,
                                 const std::vector<const vectorgpuField*>& patchSf, const scalargpuField& weights, const scalargpuField& V)
{
    const lduAddressing& a = lduAddr();
    const label n = a.size(), nI = weights.size();
    scalargpuField ssf(nI);
    miCheck(mi_face_interpolate(a.handle(), weights.data(), vf.data(), ssf.data()), "linear::interpolate");
    miCheck(mi_gauss_grad(a.handle(), Sf.component(0).data(), Sf.component(1).data(), Sf.component(2).data(), ssf.data(), nullptr,
                          g.component(0).data(), g.component(1).data(), g.component(2).data()), "gaussGrad::gradf");   // internal faces, then every patch
    for (std::size_t p = 0; p < patchFaceCells_.size(); ++p) {
        const label np = (label)patchFaceCells_[p].size();
        if (np == 0) continue;
        mi_patch_t P = patchOf(patches_, p, n, patchFaceCells_[p]);
        scalargpuField pif(np);
        const scalargpuField* pv = p < patchValues.size() ? patchValues[p] : nullptr;
        if (!pv) { miCheck(mi_patch_internal_field(P, vf.data(), pif.data()), "fvPatchField::patchInternalField"); pv = &pif; }
        for (direction d = 0; d < 3; ++d)
            miCheck(mi_patch_add_product(P, patchSf[p]->component(d).data(), pv->data(), g.component(d).data(), 0), "gaussGrad::gradf (patch)");
    }
    for (direction d = 0; d < 3; ++d) miCheck(mi_vec_div(miEngine::New().ctx, n, g.component(d).data(), V.data(), g.component(d).data()), "gaussGrad /= V");
}
void fvScalarMatrix::subtractFluxDivergence(const scalargpuField& flux, const scalargpuField& V)
{
    const lduAddressing& a = lduAddr();
    scalargpuField div(a.size());
    miCheck(mi_surface_integrate(a.handle(), flux.data(), V.data(), div.data()), "fvc::div");
    miCheck(mi_vec_submul(miEngine::New().ctx, a.size(), V.data(), div.data(), source_.data()), "fvm::laplacian: source -= V*div(correction)");
}
void fvScalarMatrix::nonOrthCorrection(const scalargpuField& vf, const std::vector<const scalargpuField*>& patchValues, const vectorgpuField& Sf,
                                       const std::vector<const vectorgpuField*>& patchSf, const scalargpuField& weights, const vectorgpuField& corrVecs,
                                       const scalargpuField& gammaMagSf, const scalargpuField& V)
{
    const lduAddressing& a = lduAddr();
    vectorgpuField g(a.size());
    gaussGradOf(g, vf, patchValues, Sf, patchSf, weights, V);
    scalargpuField flux(weights.size());
    miCheck(mi_sngrad_correction_flux(a.handle(), corrVecs.component(0).data(), corrVecs.component(1).data(), corrVecs.component(2).data(), weights.data(),
                                      g.component(0).data(), g.component(1).data(), g.component(2).data(), gammaMagSf.data(), flux.data()),
            "correctedSnGrad::correction");
    subtractFluxDivergence(flux, V);
}
void fvScalarMatrix::nonOrthCorrection(const fv::snGradScheme& scheme, const scalargpuField& vf, const std::vector<const scalargpuField*>& patchValues,
                                       const vectorgpuField& Sf, const std::vector<const vectorgpuField*>& patchSf, const scalargpuField& weights,
                                       const scalargpuField& deltaCoeffs, const vectorgpuField& corrVecs, const scalargpuField& gammaMagSf,
                                       const scalargpuField& V)
{
    if (!scheme.corrected()) return;
    if (!scheme.limited()) { nonOrthCorrection(vf, patchValues, Sf, patchSf, weights, corrVecs, gammaMagSf, V); return; }
    vectorgpuField g(lduAddr().size());
    gaussGradOf(g, vf, patchValues, Sf, patchSf, weights, V);
    scalargpuField flux(weights.size());
    fvc::snGradLimitedCorrectionFlux(flux, lduAddr(), scheme, corrVecs, weights, deltaCoeffs, vf, g, gammaMagSf);
    subtractFluxDivergence(flux, V);
}
fvScalarMatrix& fvScalarMatrix::operator+=(const fvScalarMatrix& B) { axpyFrom(B, 1.0); return *this; }
fvScalarMatrix& fvScalarMatrix::operator-=(const fvScalarMatrix& B) { axpyFrom(B, -1.0); return *this; }
fvScalarMatrix& fvScalarMatrix::operator*=(scalar s)
{
    mi_ctx_t ctx = miEngine::New().ctx;
    auto sc = [&](scalargpuField& x) { if (x.size()) miCheck(mi_vec_axpby(ctx, x.size(), s, x.data(), 0.0, x.data(), x.data()), "fvMatrix::operator*="); };
    if (asymmetric()) sc(lower());
    sc(upper()); sc(diag()); sc(source_);
    for (std::size_t p = 0; p < internalCoeffs_.size(); ++p) { sc(internalCoeffs_[p]); sc(boundaryCoeffs_[p]); }
    return *this;
}
void fvm::ddt(fvScalarMatrix& M, scalar rDeltaT, scalar rho, const scalargpuField& V, const scalargpuField& psiOld)
{
    miCheck(mi_fvm_ddt_euler(miEngine::New().ctx, V.size(), rDeltaT, rho, V.data(), psiOld.data(), M.diag().data(), M.source().data()), "fvm::ddt");
}
void fvm::assemble(fvScalarMatrix& M, scalar rDeltaT, scalar rho, const scalargpuField& V, const scalargpuField& psiOld, const scalargpuField* faceFlux,
                   const scalargpuField* weights, const scalargpuField* deltaCoeffs, const scalargpuField* gammaMagSf, const scalargpuField* su)
{
    scalargpuField* so = &M.source(); const scalargpuField* po = &psiOld;
    assembleTerms("fvm::assemble", M, &so, EulerForm(rDeltaT), rho, V, &po, 1, faceFlux, weights, deltaCoeffs, gammaMagSf, nullptr, su);
}
void fvm::assemble(fvScalarMatrix& M, scalar rDeltaT, scalar rho, const scalargpuField& V, const scalargpuField& psiOld, const scalargpuField& faceFlux,
                   const scalargpuField* weights, const scalargpuField* deltaCoeffs, const scalargpuField* gammaMagSf, const linearUpwindCorrection& corr,
                   const scalargpuField* su)
{
    scalargpuField* so = &M.source(); const scalargpuField* po = &psiOld;
    assembleTerms("fvm::assemble (corrected convection)", M, &so, EulerForm(rDeltaT), rho, V, &po, 1, &faceFlux, weights, deltaCoeffs, gammaMagSf, &corr, su);
}
void fvm::assemble(fvVectorMatrix& M, scalar rDeltaT, scalar rho, const scalargpuField& V, const vectorgpuField& psiOld, const scalargpuField& faceFlux,
                   const scalargpuField* weights, const scalargpuField* deltaCoeffs, const scalargpuField* gammaMagSf, const linearUpwindCorrection& corr)
{
    assembleTerms("fvm::assemble (corrected convection)", M, cmpts(M.source()), EulerForm(rDeltaT), rho, V, cmpts(psiOld), 3, &faceFlux, weights, deltaCoeffs,
                  gammaMagSf, &corr, nullptr);
}
// ---- the backward time scheme ----
backwardDdtCoeffs::backwardDdtCoeffs(scalar deltaT, scalar deltaT0, int nOldTimes) : rDeltaT(1.0 / deltaT)
{
    double c[3];
    miCheck(mi_ddt_backward_coeffs(deltaT, deltaT0, nOldTimes, c), "backwardDdtScheme");
    coefft = c[0]; coefft0 = c[1]; coefft00 = c[2];
}
backwardDdtCoeffs::backwardDdtCoeffs(scalar deltaT, scalar deltaT0) : backwardDdtCoeffs(deltaT, deltaT0, 2) {}
backwardDdtCoeffs backwardDdtCoeffs::firstStep(scalar deltaT) { return backwardDdtCoeffs(deltaT, 0.0, 1); }
// the terms of the Euler overloads plus the backward part (the overloads of fvm::assemble that take backwardDdtCoeffs are inline over this)
void fvm::assembleBackward(lduMatrix& M, scalargpuField* const* sources, const backwardDdtCoeffs& bd, scalar rho, const scalargpuField& V,
                      const scalargpuField* const* psiOld, const scalargpuField* const* psiOldOld, int nRhs, const scalargpuField* faceFlux,
                      const scalargpuField* weights, const scalargpuField* deltaCoeffs, const scalargpuField* gammaMagSf, const linearUpwindCorrection* corr,
                      const scalargpuField* su)
{
    assembleTerms("fvm::assemble (backward)", M, sources, {ddtForm::backward, bd.rDeltaT, &bd, 0, psiOldOld}, rho, V, psiOld, nRhs, faceFlux, weights, deltaCoeffs,
                  gammaMagSf, corr, su);
}
void fvm::ddt(fvScalarMatrix& M, const backwardDdtCoeffs& bd, scalar rho, const scalargpuField& V, const scalargpuField& psiOld, const scalargpuField& psiOldOld)
{
    const double c[3] = {bd.coefft, bd.coefft0, bd.coefft00};
    miCheck(mi_fvm_ddt_backward(miEngine::New().ctx, V.size(), bd.rDeltaT, c, rho, nullptr, nullptr, nullptr, V.data(), psiOld.data(), psiOldOld.data(),
                                M.diag().data(), M.source().data()), "fvm::ddt (backward)");
}
void fvc::ddtCorr(scalargpuField& out, const lduAddressing& a, const backwardDdtCoeffs& bd, const scalargpuField& weights, const vectorgpuField& Sf,
                  const vectorgpuField& Uold, const vectorgpuField& UoldOld, const scalargpuField& phiOld, const scalargpuField& phiOldOld)
{
    const double c[3] = {bd.coefft, bd.coefft0, bd.coefft00};
    miCheck(mi_ddt_phi_corr_backward(a.handle(), bd.rDeltaT, c, weights.data(), Sf.component(0).data(), Sf.component(1).data(), Sf.component(2).data(),
                                     Uold.component(0).data(), Uold.component(1).data(), Uold.component(2).data(), UoldOld.component(0).data(),
                                     UoldOld.component(1).data(), UoldOld.component(2).data(), nullptr, nullptr, phiOld.data(), phiOldOld.data(), out.data()),
            "fvc::ddtCorr (backward)");
}
void fvc::ddt(scalargpuField& out, const backwardDdtCoeffs& bd, const scalargpuField& vf, const scalargpuField& vfOld, const scalargpuField& vfOldOld)
{
    const double c[3] = {bd.coefft, bd.coefft0, bd.coefft00};
    miCheck(mi_fvc_ddt_backward(miEngine::New().ctx, vf.size(), bd.rDeltaT, c, 1.0, nullptr, nullptr, nullptr, vf.data(), vfOld.data(), vfOldOld.data(), out.data()),
            "fvc::ddt (backward)");
}
// ---- the CrankNicolson time scheme ----
fv::CrankNicolsonDdtScheme::CrankNicolsonDdtScheme(scalar ocCoeff) : ocCoeff_(ocCoeff), timeIndex_(0), deltaT_(0), deltaT0_(0)
{
    if (!(ocCoeff_ >= 0 && ocCoeff_ <= 1)) FatalErrorIn("CrankNicolsonDdtScheme", "coefficient = " + std::to_string(ocCoeff_) + " should be >= 0 and <= 1");
}
fv::CrankNicolsonDdtScheme fv::CrankNicolsonDdtScheme::New(const std::string& scheme)
{
    double oc = 0;
    miCheck(mi_ddt_cn_parse(scheme.c_str(), &oc), "ddtSchemes");
    return CrankNicolsonDdtScheme(oc);
}
fv::CrankNicolsonDdtScheme::DDt0Field& fv::CrankNicolsonDdtScheme::lookup(const word& name, label nCells, int nCmpt)
{
    if (nCmpt < 1 || nCmpt > 4) FatalErrorIn("CrankNicolsonDdtScheme", name + ": 1 to 4 components, " + std::to_string(nCmpt) + " given");
    auto it = ddt0_.find(name);
    if (it == ddt0_.end()) {                          // created zero, with the current time index as its own and as its start
        DDt0Field f;
        miCheck(mi_ddt_cn_begin(ocCoeff_, timeIndex_, &f.state), "CrankNicolsonDdtScheme");
        for (int k = 0; k < nCmpt; ++k) f.cmpt.emplace_back(nCells);
        it = ddt0_.emplace(name, std::move(f)).first;
    }
    if ((int)it->second.cmpt.size() != nCmpt || it->second.cmpt[0].size() != nCells)
        FatalErrorIn("CrankNicolsonDdtScheme", name + ": used with another size or number of components than it was created with");
    return it->second;
}
const scalargpuField& fv::CrankNicolsonDdtScheme::ddt0(const word& name, direction cmpt) const
{
    auto it = ddt0_.find(name);
    if (it == ddt0_.end() || cmpt >= it->second.cmpt.size()) FatalErrorIn("CrankNicolsonDdtScheme", "no field " + name);
    return it->second.cmpt[cmpt];
}
scalar fv::CrankNicolsonDdtScheme::evaluate(const word& name, scalar rho, const scalargpuField* const* psiOld, const scalargpuField* const* psiOldOld, int nCmpt)
{
    if (nCmpt < 1 || nCmpt > 4 || !psiOld || !psiOldOld) FatalErrorIn("CrankNicolsonDdtScheme", name + ": 1 to 4 components with their old and old-old fields");
    for (int k = 0; k < nCmpt; ++k) if (!psiOld[k] || !psiOldOld[k]) FatalErrorIn("CrankNicolsonDdtScheme", name + ": a missing old or old-old field");
    DDt0Field& f = lookup(name, psiOld[0]->size(), nCmpt);
    mi_ddt_cn_scalars sc{};
    miCheck(mi_ddt_cn_step(&f.state, timeIndex_, deltaT_, deltaT0_, &sc), "CrankNicolsonDdtScheme");
    if (sc.evaluate) {
        const double *po[4], *poo[4]; double* d[4];
        for (int k = 0; k < nCmpt; ++k) { po[k] = psiOld[k]->data(); poo[k] = psiOldOld[k]->data(); d[k] = f.cmpt[k].data(); }
        miCheck(mi_ddt_cn_update(miEngine::New().ctx, psiOld[0]->size(), nCmpt, sc.r_dt_coef0, ocCoeff_, rho, nullptr, nullptr, po, poo, d), name.c_str());
    }
    return sc.r_dt_coef;
}
scalar fv::CrankNicolsonDdtScheme::rDtCoef(const word& name, label nCells, int nCmpt)
{
    mi_ddt_cn_state probe = lookup(name, nCells, nCmpt).state;   // stepped on a COPY: the field's own time index stays, ddt0 is not due an update
    mi_ddt_cn_scalars sc{};
    miCheck(mi_ddt_cn_step(&probe, timeIndex_, deltaT_, deltaT0_ > 0 ? deltaT0_ : deltaT_, &sc), "CrankNicolsonDdtScheme");   // only r_dt_coef is used
    return sc.r_dt_coef;
}
void fv::CrankNicolsonDdtScheme::assemble(lduMatrix& M, scalargpuField* const* sources, const word& name, scalar rho, const scalargpuField& V,
                                          const scalargpuField* const* psiOld, const scalargpuField* const* psiOldOld, int nRhs, const scalargpuField* faceFlux,
                                          const scalargpuField* weights, const scalargpuField* deltaCoeffs, const scalargpuField* gammaMagSf,
                                          const linearUpwindCorrection* corr, const scalargpuField* su)
{
    if (nRhs < 1 || nRhs > 3 || !sources) FatalErrorIn("fvm::assemble (CrankNicolson)", name + ": 1 to 3 right-hand sides, " + std::to_string(nRhs) + " given");
    for (int r = 0; r < nRhs; ++r) if (!sources[r]) FatalErrorIn("fvm::assemble (CrankNicolson)", name + ": a missing source field");
    const scalar rDtCoef = evaluate(name, rho, psiOld, psiOldOld, nRhs);
    const scalargpuField* d0[3];
    for (int r = 0; r < nRhs; ++r) d0[r] = &ddt0(name, r);
    assembleTerms("fvm::assemble (CrankNicolson)", M, sources, {ddtForm::CrankNicolson, rDtCoef, nullptr, ocCoeff_, d0}, rho, V, psiOld, nRhs, faceFlux, weights,
                  deltaCoeffs, gammaMagSf, corr, su);
}
void fvm::ddt(fvScalarMatrix& M, fv::CrankNicolsonDdtScheme& cn, const word& name, scalar rho, const scalargpuField& V, const scalargpuField& psiOld,
              const scalargpuField& psiOldOld)
{
    const scalargpuField *po[1] = {&psiOld}, *poo[1] = {&psiOldOld};
    const scalar rDtCoef = cn.evaluate(name, rho, po, poo, 1);
    miCheck(mi_fvm_ddt_cn(miEngine::New().ctx, V.size(), rDtCoef, cn.ocCoeff(), rho, nullptr, nullptr, V.data(), psiOld.data(), cn.ddt0(name).data(),
                          M.diag().data(), M.source().data()), "fvm::ddt (CrankNicolson)");
}
void fvc::ddtCorr(scalargpuField& out, const lduAddressing& a, fv::CrankNicolsonDdtScheme& cn, const word& name, const scalargpuField& weights,
                  const vectorgpuField& Sf, const vectorgpuField& Uold, const scalargpuField& phiOld)
{
    fvc::ddtCorr(out, a, cn.rDtCoef(name, Uold.component(0).size(), 3), weights, Sf, Uold, phiOld);
}
void fvc::ddt(scalargpuField& out, fv::CrankNicolsonDdtScheme& cn, const word& name, const scalargpuField& vf, const scalargpuField& vfOld,
              const scalargpuField& vfOldOld)
{
    const scalargpuField *po[1] = {&vfOld}, *poo[1] = {&vfOldOld};
    const scalar rDtCoef = cn.evaluate(name, 1.0, po, poo, 1);
    miCheck(mi_fvc_ddt_cn(miEngine::New().ctx, vf.size(), rDtCoef, cn.ocCoeff(), 1.0, nullptr, nullptr, vf.data(), vfOld.data(), cn.ddt0(name).data(), out.data()),
            "fvc::ddt (CrankNicolson)");
}
void fvc::linearUpwindCorrectionFlux(scalargpuField& out, const lduAddressing& a, const scalargpuField& faceFlux, const linearUpwindCorrection& corr)
{
    const mi_div_correction k = divCorrection(corr, 1);
    double* o[1] = {out.data()};
    miCheck(mi_linear_upwind_correction(a.handle(), &k, 1, faceFlux.data(), o), "linearUpwind::correction");
}
void fvc::linearUpwindCorrectionFlux(vectorgpuField& out, const lduAddressing& a, const scalargpuField& faceFlux, const linearUpwindCorrection& corr)
{
    const mi_div_correction k = divCorrection(corr, 3);
    const auto o = cmptData(out);
    miCheck(mi_linear_upwind_correction(a.handle(), &k, 3, faceFlux.data(), o), "linearUpwind::correction");
}
namespace {
mi_cubic_geometry cubicGeometry(const scalargpuField& lambda, const vectorgpuField& Sf, const scalargpuField& magSf, const scalargpuField& deltaCoeffs)
{
    mi_cubic_geometry g{};
    g.lambda_dev = lambda.data(); g.mag_sf_dev = magSf.data(); g.delta_coeffs_dev = deltaCoeffs.data();
    for (int d = 0; d < 3; ++d) g.sf_dev[d] = Sf.component(d).data();
    return g;
}
}
void fvc::cubicCorrectionFlux(scalargpuField& out, const lduAddressing& a, const scalargpuField* faceFlux, const scalargpuField& lambda, const vectorgpuField& Sf,
                              const scalargpuField& magSf, const scalargpuField& deltaCoeffs, const scalargpuField& vf, const vectorgpuField& gradVf)
{
    const mi_cubic_geometry geo = cubicGeometry(lambda, Sf, magSf, deltaCoeffs);
    const double* v[1] = {vf.data()};
    const auto g = cmptData(gradVf);
    double* o[1] = {out.data()};
    miCheck(mi_cubic_correction(a.handle(), &geo, 1, v, g, faceFlux ? faceFlux->data() : nullptr, o), "cubic::correction");
}
void fvc::cubicCorrectionFlux(vectorgpuField& out, const lduAddressing& a, const scalargpuField* faceFlux, const scalargpuField& lambda, const vectorgpuField& Sf,
                              const scalargpuField& magSf, const scalargpuField& deltaCoeffs, const vectorgpuField& vf, const vectorgpuField* const gradVf[3])
{
    const mi_cubic_geometry geo = cubicGeometry(lambda, Sf, magSf, deltaCoeffs);
    const double *v[3], *g[9];
    double* o[3];
    for (int j = 0; j < 3; ++j) {
        v[j] = vf.component(j).data(); o[j] = out.component(j).data();
        for (int d = 0; d < 3; ++d) g[3 * j + d] = gradVf[j]->component(d).data();
    }
    miCheck(mi_cubic_correction(a.handle(), &geo, 3, v, g, faceFlux ? faceFlux->data() : nullptr, o), "cubic::correction");
}
void fvc::grad(vectorgpuField& g, const lduAddressing& a, const vectorgpuField& Sf, const scalargpuField& ssf, const scalargpuField& V)
{
    miCheck(mi_gauss_grad(a.handle(), Sf.component(0).data(), Sf.component(1).data(), Sf.component(2).data(), ssf.data(), V.data(),
                          g.component(0).data(), g.component(1).data(), g.component(2).data()), "fvc::grad");
}
void fvc::interpolate(scalargpuField& sf, const lduAddressing& a, const scalargpuField& weights, const scalargpuField& vf)
{
    miCheck(mi_face_interpolate(a.handle(), weights.data(), vf.data(), sf.data()), "fvc::interpolate");
}
void fvc::surfaceIntegrate(scalargpuField& ivf, const lduAddressing& a, const scalargpuField& ssf, const scalargpuField* V)
{
    miCheck(mi_surface_integrate(a.handle(), ssf.data(), V ? V->data() : nullptr, ivf.data()), "fvc::surfaceIntegrate");
}
void fvc::fluxDiv(scalargpuField& phi, scalargpuField* divOut, const lduAddressing& a, const scalargpuField& weights, const vectorgpuField& Sf,
                  const vectorgpuField& Vf, const scalargpuField* addA, const scalargpuField* addB, const scalargpuField* V)
{
    scalargpuField scratch(divOut ? 0 : a.size());
    miCheck(mi_flux_div(a.handle(), weights.data(), Sf.component(0).data(), Sf.component(1).data(), Sf.component(2).data(),
                        Vf.component(0).data(), Vf.component(1).data(), Vf.component(2).data(), nullptr, addA ? addA->data() : nullptr,
                        addB ? addB->data() : nullptr, phi.data(), V ? V->data() : nullptr, divOut ? divOut->data() : scratch.data()), "fvc::flux + fvc::div");
}
void fvc::snGradCorrectionFlux(scalargpuField& flux, const lduAddressing& a, const vectorgpuField& corrVecs, const scalargpuField& weights,
                               const vectorgpuField& gradVf, const scalargpuField& gammaMagSf)
{
    miCheck(mi_sngrad_correction_flux(a.handle(), corrVecs.component(0).data(), corrVecs.component(1).data(), corrVecs.component(2).data(), weights.data(),
                                      gradVf.component(0).data(), gradVf.component(1).data(), gradVf.component(2).data(), gammaMagSf.data(), flux.data()),
            "correctedSnGrad::correction");
}
void fvc::ddtCorr(scalargpuField& out, const lduAddressing& a, scalar rDeltaT, const scalargpuField& weights, const vectorgpuField& Sf,
                  const vectorgpuField& Uold, const scalargpuField& phiOld)
{
    miCheck(mi_ddt_phi_corr(a.handle(), rDeltaT, weights.data(), Sf.component(0).data(), Sf.component(1).data(), Sf.component(2).data(),
                            Uold.component(0).data(), Uold.component(1).data(), Uold.component(2).data(), nullptr, phiOld.data(), out.data()), "fvc::ddtCorr");
}
void fieldAxpby(scalargpuField& out, scalar a, const scalargpuField& x, scalar b, const scalargpuField& y)
{
    miCheck(mi_vec_axpby(miEngine::New().ctx, out.size(), a, x.data(), b, y.data(), out.data()), "gpuField: a x + b y");
}
void fieldDivide(scalargpuField& out, const scalargpuField& x, const scalargpuField& y)
{
    miCheck(mi_vec_div(miEngine::New().ctx, out.size(), x.data(), y.data(), out.data()), "gpuField: x / y");
}
void fieldSubMul(scalargpuField& inout, const scalargpuField& x, const scalargpuField& y)
{
    miCheck(mi_vec_submul(miEngine::New().ctx, inout.size(), x.data(), y.data(), inout.data()), "gpuField: -= x*y");
}
fvPatchCells::fvPatchCells(label nCells, const labelList& faceCells) : h_(nullptr), n_((label)faceCells.size())
{
    miCheck(mi_patch_create(miEngine::New().ctx, nCells, n_, faceCells.data(), &h_), "fvPatch::faceCells");
}
fvPatchCells::~fvPatchCells() { if (h_) mi_patch_destroy(h_); }
void fvPatchCells::add(const scalargpuField& pf, scalargpuField& intf, bool subtract) const
{
    if (n_) miCheck(mi_patch_add(h_, pf.data(), intf.data(), subtract ? 1 : 0), "fvPatch: cells += patch field");
}
void fvPatchCells::addProduct(const scalargpuField& pf, const scalargpuField& q, scalargpuField& intf, bool subtract) const
{
    if (n_) miCheck(mi_patch_add_product(h_, pf.data(), q.data(), intf.data(), subtract ? 1 : 0), "fvPatch: cells += patch field * patch field");
}
void fvPatchCells::patchInternalField(const scalargpuField& psi, scalargpuField& out) const
{
    if (n_) miCheck(mi_patch_internal_field(h_, psi.data(), out.data()), "fvPatchField::patchInternalField");
}
void upwindWeights(scalargpuField& w, const scalargpuField& faceFlux)
{
    miCheck(mi_upwind_weights(miEngine::New().ctx, faceFlux.size(), faceFlux.data(), w.data()), "upwind::weights");
}
void LUSTWeights(scalargpuField& w, const scalargpuField& cdWeights, const scalargpuField& faceFlux)
{
    miCheck(mi_lust_weights(miEngine::New().ctx, faceFlux.size(), cdWeights.data(), faceFlux.data(), w.data()), "LUST::weights");
}
void limitedLinearWeights(scalargpuField& w, const lduAddressing& a, scalar k, const scalargpuField& cdWeights, const scalargpuField& faceFlux,
                          const scalargpuField& vf, const vectorgpuField& gradVf, const vectorgpuField& C)
{
    miCheck(mi_limited_linear_weights(a.handle(), k, cdWeights.data(), faceFlux.data(), vf.data(), gradVf.component(0).data(),
                                      gradVf.component(1).data(), gradVf.component(2).data(), C.component(0).data(), C.component(1).data(),
                                      C.component(2).data(), w.data(), nullptr), "limitedLinear::weights");
}

limitedScheme limitedScheme::New(const std::string& scheme)
{
    mi_limiter l{};
    miCheck(mi_limiter_parse(scheme.c_str(), &l), "limitedSurfaceInterpolationScheme::New");
    return limitedScheme(l);
}
namespace {
struct limitedArrays
{
    const double* phi[3]; const double* grad[9]; int m = 0;
    limitedArrays(const scalargpuField& vf, const vectorgpuField& g) : m(1)
    {
        phi[0] = vf.data();
        for (int k = 0; k < 3; ++k) grad[k] = g.component(k).data();
    }
    limitedArrays(const vectorgpuField& vf, const vectorgpuField* const g[3]) : m(3)
    {
        for (int j = 0; j < 3; ++j) {
            phi[j] = vf.component(j).data();
            for (int k = 0; k < 3; ++k) grad[3 * j + k] = g[j]->component(k).data();
        }
    }
};
const double* const* comps(const vectorgpuField& v, const double* (&out)[3])
{
    for (int k = 0; k < 3; ++k) out[k] = v.component(k).data();
    return out;
}
void limitedCall(scalargpuField& w, const lduAddressing& a, const limitedScheme& s, const scalargpuField& cdWeights, const scalargpuField& faceFlux,
                 const limitedArrays& q, const vectorgpuField& C, scalargpuField* limiter)
{
    const double* c[3];
    miCheck(mi_limited_weights(a.handle(), &s.data(), cdWeights.data(), faceFlux.data(), q.phi, q.grad, comps(C, c), w.data(),
                               limiter ? limiter->data() : nullptr), "LimitedScheme::weights");
}
void patchLimitedCall(scalargpuField& w, const fvPatchCells& p, const limitedScheme& s, const scalargpuField& pCdWeights, const scalargpuField& pFaceFlux,
                      const limitedArrays& own, const limitedArrays& nbr, const vectorgpuField& pDelta, scalargpuField* limiter)
{
    const double* d[3];
    miCheck(mi_patch_limited_weights(p.handle(), &s.data(), pCdWeights.data(), pFaceFlux.data(), own.phi, nbr.phi, own.grad, nbr.grad,
                                     comps(pDelta, d), w.data(), limiter ? limiter->data() : nullptr), "LimitedScheme::weights (coupled patch)");
}
} // namespace
void limitedWeights(scalargpuField& w, const lduAddressing& a, const limitedScheme& s, const scalargpuField& cdWeights, const scalargpuField& faceFlux,
                    const scalargpuField& vf, const vectorgpuField& gradVf, const vectorgpuField& C, scalargpuField* limiter)
{
    limitedCall(w, a, s, cdWeights, faceFlux, limitedArrays(vf, gradVf), C, limiter);
}
void limitedWeights(scalargpuField& w, const lduAddressing& a, const limitedScheme& s, const scalargpuField& cdWeights, const scalargpuField& faceFlux,
                    const vectorgpuField& vf, const vectorgpuField* const gradVf[3], const vectorgpuField& C, scalargpuField* limiter)
{
    limitedCall(w, a, s, cdWeights, faceFlux, limitedArrays(vf, gradVf), C, limiter);
}
void patchLimitedWeights(scalargpuField& w, const fvPatchCells& p, const limitedScheme& s, const scalargpuField& pCdWeights, const scalargpuField& pFaceFlux,
                         const scalargpuField& vf, const scalargpuField& nbrVf, const vectorgpuField& gradVf, const vectorgpuField& nbrGradVf,
                         const vectorgpuField& pDelta, scalargpuField* limiter)
{
    patchLimitedCall(w, p, s, pCdWeights, pFaceFlux, limitedArrays(vf, gradVf), limitedArrays(nbrVf, nbrGradVf), pDelta, limiter);
}
void patchLimitedWeights(scalargpuField& w, const fvPatchCells& p, const limitedScheme& s, const scalargpuField& pCdWeights, const scalargpuField& pFaceFlux,
                         const vectorgpuField& vf, const vectorgpuField& nbrVf, const vectorgpuField* const gradVf[3],
                         const vectorgpuField* const nbrGradVf[3], const vectorgpuField& pDelta, scalargpuField* limiter)
{
    patchLimitedCall(w, p, s, pCdWeights, pFaceFlux, limitedArrays(vf, gradVf), limitedArrays(nbrVf, nbrGradVf), pDelta, limiter);
}

filteredScheme filteredScheme::New(const std::string& scheme)
{
    mi_filtered_limiter l{};
    miCheck(mi_filtered_parse(scheme.c_str(), &l), "limitedSurfaceInterpolationScheme::New");
    return filteredScheme(l);
}
namespace {
void filteredCall(scalargpuField& w, const lduAddressing& a, const filteredScheme& s, const scalargpuField& cdWeights, const scalargpuField& faceFlux,
                  const limitedArrays& q, const vectorgpuField& C, scalargpuField* limiter)
{
    const double* c[3];
    miCheck(mi_filtered_weights(a.handle(), &s.data(), cdWeights.data(), faceFlux.data(), q.phi, q.grad, comps(C, c), w.data(),
                                limiter ? limiter->data() : nullptr), "LimitedScheme::weights (filtered)");
}
void patchFilteredCall(scalargpuField& w, const fvPatchCells& p, const filteredScheme& s, const scalargpuField& pCdWeights, const scalargpuField& pFaceFlux,
                       const limitedArrays& own, const limitedArrays& nbr, const vectorgpuField& pDelta, scalargpuField* limiter)
{
    const double* d[3];
    miCheck(mi_patch_filtered_weights(p.handle(), &s.data(), pCdWeights.data(), pFaceFlux.data(), own.phi, nbr.phi, own.grad, nbr.grad,
                                      comps(pDelta, d), w.data(), limiter ? limiter->data() : nullptr), "LimitedScheme::weights (filtered, coupled patch)");
}
} // namespace
void filteredWeights(scalargpuField& w, const lduAddressing& a, const filteredScheme& s, const scalargpuField& cdWeights, const scalargpuField& faceFlux,
                     const scalargpuField& vf, const vectorgpuField& gradVf, const vectorgpuField& C, scalargpuField* limiter)
{
    filteredCall(w, a, s, cdWeights, faceFlux, limitedArrays(vf, gradVf), C, limiter);
}
void filteredWeights(scalargpuField& w, const lduAddressing& a, const filteredScheme& s, const scalargpuField& cdWeights, const scalargpuField& faceFlux,
                     const vectorgpuField& vf, const vectorgpuField* const gradVf[3], const vectorgpuField& C, scalargpuField* limiter)
{
    filteredCall(w, a, s, cdWeights, faceFlux, limitedArrays(vf, gradVf), C, limiter);
}
void patchFilteredWeights(scalargpuField& w, const fvPatchCells& p, const filteredScheme& s, const scalargpuField& pCdWeights, const scalargpuField& pFaceFlux,
                          const scalargpuField& vf, const scalargpuField& nbrVf, const vectorgpuField& gradVf, const vectorgpuField& nbrGradVf,
                          const vectorgpuField& pDelta, scalargpuField* limiter)
{
    patchFilteredCall(w, p, s, pCdWeights, pFaceFlux, limitedArrays(vf, gradVf), limitedArrays(nbrVf, nbrGradVf), pDelta, limiter);
}
void patchFilteredWeights(scalargpuField& w, const fvPatchCells& p, const filteredScheme& s, const scalargpuField& pCdWeights, const scalargpuField& pFaceFlux,
                          const vectorgpuField& vf, const vectorgpuField& nbrVf, const vectorgpuField* const gradVf[3],
                          const vectorgpuField* const nbrGradVf[3], const vectorgpuField& pDelta, scalargpuField* limiter)
{
    patchFilteredCall(w, p, s, pCdWeights, pFaceFlux, limitedArrays(vf, gradVf), limitedArrays(nbrVf, nbrGradVf), pDelta, limiter);
}

interfaceCompressionScheme interfaceCompressionScheme::New(const std::string& scheme)
{
    miCheck(mi_interface_compression_parse(scheme.c_str()), "limitedSurfaceInterpolationScheme::New");
    return interfaceCompressionScheme();
}
void interfaceCompressionWeights(scalargpuField& w, const lduAddressing& a, const interfaceCompressionScheme&, const scalargpuField& cdWeights,
                                 const scalargpuField& faceFlux, const scalargpuField& vf, scalargpuField* limiter)
{
    miCheck(mi_interface_compression_weights(a.handle(), cdWeights.data(), faceFlux.data(), vf.data(), w.data(), limiter ? limiter->data() : nullptr),
            "PhiScheme::weights");
}
void patchInterfaceCompressionWeights(scalargpuField& w, const fvPatchCells& p, const interfaceCompressionScheme&, const scalargpuField& pCdWeights,
                                      const scalargpuField& pFaceFlux, const scalargpuField& vf, const scalargpuField& nbrVf, scalargpuField* limiter)
{
    miCheck(mi_patch_interface_compression_weights(p.handle(), pCdWeights.data(), pFaceFlux.data(), vf.data(), nbrVf.data(), w.data(),
                                                   limiter ? limiter->data() : nullptr), "PhiScheme::weights (coupled patch)");
}
void alphaCompressionFlux(scalargpuField& flux, const lduAddressing& a, const interfaceCompressionScheme&, const scalargpuField& cdWeights,
                          const scalargpuField& phir, const scalargpuField& alpha1)
{
    miCheck(mi_alpha_compression_flux(a.handle(), cdWeights.data(), phir.data(), alpha1.data(), flux.data()), "alphaCompressionFlux");
}
void patchAlphaCompressionFlux(scalargpuField& flux, const fvPatchCells& p, const interfaceCompressionScheme&, const scalargpuField& pCdWeights,
                               const scalargpuField& pPhir, const scalargpuField& alpha1, const scalargpuField& nbrAlpha1)
{
    miCheck(mi_patch_alpha_compression_flux(p.handle(), pCdWeights.data(), pPhir.data(), alpha1.data(), nbrAlpha1.data(), flux.data()),
            "alphaCompressionFlux (coupled patch)");
}

// ---- interfaceProperties (interfaceProperties.C:58-231) ---------------------------------------------------------
namespace {
label interfaceBoundaryFaces(const std::vector<interfaceProperties::patchData>& patches)
{
    label n = 0;
    for (const auto& p : patches) n += p.cells->size();
    return n;
}
}
interfaceProperties::interfaceProperties(const meshData& mesh, const std::vector<patchData>& patches, scalar cAlpha, scalar sigma)
    : mesh_(mesh), patches_(patches), cAlpha_(cAlpha), sigma_(sigma), deltaN_(0), h_(nullptr),
      nHatf_((label)mesh.addr->lowerAddrHost().size()), nHatfb_(interfaceBoundaryFaces(patches)), K_(mesh.V->size())
{
    // deltaN_("deltaN", 1e-8/pow(average(alpha1.mesh().V()), 1.0/3.0)) (:181-185): the sum on the host in cell order
    const std::vector<scalar> V = mesh.V->asHost();
    scalar s = 0;
    for (scalar v : V) s += v;
    deltaN_ = 1e-8 / std::pow(s / (scalar)V.size(), 1.0 / 3.0);
    miCheck(mi_interface_create(mesh.addr->handle(), mesh.boundary ? mesh.boundary->handle() : nullptr, &h_), "interfaceProperties::New");
}
interfaceProperties::~interfaceProperties() { if (h_) mi_interface_destroy(h_); }
averageData::averageData(const lduAddressing& a, const gradBoundary* b, const scalargpuField& magSf, const scalargpuField* bMagSf)
    : h_(nullptr), magSf_(&magSf), bMagSf_(bMagSf)
{
    miCheck(mi_average_create(a.handle(), b ? b->handle() : nullptr, magSf.data(), bMagSf ? bMagSf->data() : nullptr, &h_), "averageData::New");
}
averageData::~averageData() { if (h_) mi_average_destroy(h_); }
void fvc::average(scalargpuField& out, const averageData& av, const scalargpuField& ssf, const scalargpuField* bssf)
{
    miCheck(mi_fvc_average(av.handle(), av.magSf().data(), av.bMagSf() ? av.bMagSf()->data() : nullptr, ssf.data(), bssf ? bssf->data() : nullptr,
                           out.data()), "fvc::average");
}
bool bound(scalargpuField& vsf, scalargpuField* bvsf, const averageData& av, const scalargpuField& weights, scalar lowerBound)
{
    const mi_ctx_t ctx = miEngine::New().ctx;
    scalar minVsf = 0, minB = 0;
    miCheck(mi_min_max(ctx, vsf.size(), vsf.data(), &minVsf, nullptr), "bound");
    miCheck(mi_min_max(ctx, bvsf ? bvsf->size() : 0, bvsf ? bvsf->data() : nullptr, &minB, nullptr), "bound");   // no faces: +inf
    if (!(std::min(minVsf, minB) < lowerBound)) return false;
    if (bvsf) miCheck(mi_vec_max_value(ctx, bvsf->size(), bvsf->data(), lowerBound, bvsf->data()), "bound");
    miCheck(mi_bound(av.handle(), lowerBound, weights.data(), av.magSf().data(), av.bMagSf() ? av.bMagSf()->data() : nullptr,
                     bvsf ? bvsf->data() : nullptr, vsf.data()), "bound");
    return true;
}

// ---- incompressible::RASModels::kEpsilon ------------------------------------------------------------------------------------------------
namespace incompressible
{
namespace RASModels
{
kEpsilon::kEpsilon(const meshData& mesh, scalar nu, const scalargpuField& k, const scalargpuField& bk, const scalargpuField& epsilon,
                   const scalargpuField& bepsilon, const dictionary& coeffDict, scalar kMin, scalar epsilonMin)
    : mesh_(mesh), nu_(nu), kMin_(kMin), epsilonMin_(epsilonMin), h_(nullptr), nb_(bk.size()), k_(k), epsilon_(epsilon), nut_(k.size()), bk_(bk),
      bepsilon_(bepsilon), bnut_(bk.size()), bnu_(std::vector<scalar>((std::size_t)bk.size(), nu))
{
    const char* who = "kEpsilon::New";
    if (!mesh.addr || !mesh.boundary || !mesh.average) FatalErrorIn(who, "the addressing, the boundary and the averageData are needed");
    if (mesh.patchTypes.size() != mesh.patchFaceCells.size()) FatalErrorIn(who, "one type per patch");
    scalar Cmu = 0.09, C1 = 1.44, C2 = 1.92, sigmaEps = 1.3, kappa = 0.41, E = 9.8;      // kEpsilon.C:50-86, nutWallFunction's kappa and E
    coeffDict.readIfPresent("Cmu", Cmu); coeffDict.readIfPresent("C1", C1); coeffDict.readIfPresent("C2", C2);
    coeffDict.readIfPresent("sigmaEps", sigmaEps); coeffDict.readIfPresent("kappa", kappa); coeffDict.readIfPresent("E", E);
    miCheck(mi_ke_coeffs_init(Cmu, C1, C2, sigmaEps, kappa, E, &coeffs_), who);
    std::vector<int32_t> wall;
    label off = 0;
    for (std::size_t p = 0; p < mesh.patchFaceCells.size(); ++p) {
        wall.push_back(mesh.patchTypes[p] == wallFunction ? 1 : 0);
        start_.push_back(off);
        patches_.emplace_back(new fvPatchCells(mesh.addr->size(), mesh.patchFaceCells[p]));
        off += (label)mesh.patchFaceCells[p].size();
    }
    start_.push_back(off);
    if (off != nb_ || bepsilon.size() != nb_) FatalErrorIn(who, "the boundary fields do not have one value per boundary face");
    miCheck(mi_ke_create(mesh.addr->handle(), mesh.boundary->handle(), wall.data(), &h_), who);
    int32_t nWall = 0; const int32_t* labels = nullptr;
    miCheck(mi_ke_wall_cell_labels(h_, &nWall, &labels), who);
    labelgpuList cells(nWall);
    if (nWall) miCopyD2D(cells.data(), labels, sizeof(label) * (std::size_t)nWall);
    wallCells_.swap(cells);
    bound(k_, &bk_, *mesh_.average, *mesh_.weights, kMin_);                  // :132
    bound(epsilon_, &bepsilon_, *mesh_.average, *mesh_.weights, epsilonMin_); // :133
    correctNut();                                                            // :135-136
}
kEpsilon::~kEpsilon() { if (h_) mi_ke_destroy(h_); }
void kEpsilon::correctNut()
{
    const mi_ctx_t ctx = miEngine::New().ctx;
    miCheck(mi_ke_nut(ctx, k_.size(), coeffs_.Cmu, k_.data(), epsilon_.data(), nut_.data()), "kEpsilon: nut");
    miCheck(mi_ke_nut(ctx, nb_, coeffs_.Cmu, bk_.data(), bepsilon_.data(), bnut_.data()), "kEpsilon: nut");
    miCheck(mi_ke_nut_wall(h_, &coeffs_, k_.data(), mesh_.y->data(), bnu_.data(), bnut_.data(), nullptr), "nutkWallFunction::calcNut");
}
void kEpsilon::evaluateBoundary(const scalargpuField& vf, scalargpuField& bvf) const
{
    for (std::size_t p = 0; p < patches_.size(); ++p)
        if (mesh_.patchTypes[p] != fixedValue && patches_[p]->size() > 0)
            miCheck(mi_patch_internal_field(patches_[p]->handle(), vf.data(), bvf.data() + start_[p]), "fvPatchField::evaluate");
}
void kEpsilon::nuEff(scalargpuField& out) const { DkEff(out); }
void kEpsilon::DkEff(scalargpuField& out) const
{
    scalargpuField sp(k_.size());
    miCheck(mi_ke_k_terms(miEngine::New().ctx, k_.size(), epsilon_.data(), k_.data(), nut_.data(), nullptr, nu_, sp.data(), out.data()), "kEpsilon::DkEff");
}
void kEpsilon::DepsilonEff(scalargpuField& out) const
{
    scalargpuField su(k_.size()), sp(k_.size());
    miCheck(mi_ke_epsilon_terms(miEngine::New().ctx, k_.size(), &coeffs_, nut_.data(), epsilon_.data(), k_.data(), nut_.data(), nullptr, nu_, su.data(),
                                sp.data(), out.data()), "kEpsilon::DepsilonEff");
}
void kEpsilon::divDevReff(fvVectorMatrix& UEqn, const vectorgpuField& Sf, const vectorgpuField* const gradU[3],
                          const std::vector<fvc::devTGradPatch>& patches) const
{
    scalargpuField visc(k_.size());
    nuEff(visc);
    vectorgpuField div(k_.size());
    fvc::divDevTGrad(div, *mesh_.addr, fvc::DEV, *mesh_.weights, Sf, visc, gradU, patches, *mesh_.V);
    UEqn.subtractField(div, *mesh_.V);
}
solverPerformance kEpsilon::solveEquation(const word& name, scalargpuField& psi, const scalargpuField& bpsi, const scalargpuField& psiOld,
                                          const scalargpuField& su, const scalargpuField& sp, const scalargpuField& gamma, scalar bGammaDivisor,
                                          const flowData& flow, scalar rDeltaT, scalar alpha, bool manipulate, const dictionary& solverControls)
{
#pragma clang fp contract(off)
    const lduAddressing& a = *mesh_.addr;
    const label nf = mesh_.magSf->size();
    // gammaMagSf = fvc::interpolate(gamma)*magSf: 0 - f*magSf, then the exact negation
    scalargpuField f(nf), gammaMagSf(nf);
    fvc::interpolate(f, a, *mesh_.weights, gamma);
    fieldSubMul(gammaMagSf, f, *mesh_.magSf);
    fieldAxpby(gammaMagSf, -1.0, gammaMagSf, 0.0, gammaMagSf);
    std::vector<bool> coupled(mesh_.patchFaceCells.size(), false);
    fvScalarMatrix M(name, a, mesh_.patchFaceCells, coupled);
    mi_fvm_terms t{};
    const double* po[1] = {psiOld.data()}; const double* sd[1] = {su.data()}; const double sg[1] = {-1.0}; double* so[1] = {M.source().data()};
    t.ddt = 1; t.r_delta_t = rDeltaT; t.rho_value = 1.0; t.vol_dev = mesh_.V->data();
    t.div_flux_dev = flow.phi->data(); t.div_weights_dev = (flow.divWeights ? flow.divWeights : mesh_.weights)->data();
    t.lap_delta_coeffs_dev = mesh_.deltaCoeffs->data(); t.lap_gamma_magsf_dev = gammaMagSf.data();
    t.sp_dev = sp.data(); t.sp_sign = 1.0;                  // == ... - fvm::Sp(sp, psi): diag += V*sp
    t.n_rhs = 1; t.psi_old_dev = po; t.n_su = 1; t.su_dev = sd; t.su_sign = sg;   // == su: source += V*su
    miCheck(mi_fvm_assemble(a.handle(), &t, M.lower().data(), M.upper().data(), M.diag().data(), so, nullptr), "kEpsilon: fvm::assemble");
    // the patches: fixedValue: the diffusion coefficient and (diff - phi)*value; zeroGradient and the wall functions: the flux and nothing.
    // The boundary value of gamma is nut/divisor + nu
    const std::vector<scalar> bnut = bnut_.asHost(), bms = mesh_.bMagSf->asHost(), bdc = mesh_.bDeltaCoeffs->asHost(), bphi = flow.bPhi->asHost(),
                              bval = bpsi.asHost();
    for (std::size_t p = 0; p < patches_.size(); ++p) {
        const label m = start_[p + 1] - start_[p];
        std::vector<scalar> ic((std::size_t)m), bc((std::size_t)m);
        for (label i = 0; i < m; ++i) {
            const std::size_t j = (std::size_t)(start_[p] + i);
            if (mesh_.patchTypes[p] == fixedValue) {
                const scalar q = bnut[j] / bGammaDivisor, g = q + nu_, gm = g * bms[j], diff = gm * bdc[j];
                const scalar x = diff * bval[j], y = bphi[j] * bval[j];
                ic[(std::size_t)i] = diff; bc[(std::size_t)i] = x - y;
            } else { ic[(std::size_t)i] = bphi[j]; bc[(std::size_t)i] = 0.0; }
        }
        M.internalCoeffs()[p] = ic; M.boundaryCoeffs()[p] = bc;
    }
    M.relax(alpha, psi);
    if (manipulate && wallCells_.size() > 0) {               // boundaryManipulate: epsilonWallFunction::manipulateMatrix
        scalargpuField values(wallCells_.size());
        miCheck(mi_ke_wall_values(h_, psi.data(), values.data()), "epsilonWallFunction::manipulateMatrix");
        M.setValues(wallCells_, values, psi);
    }
    return M.solve(psi, solverControls);
}
void kEpsilon::correct(const flowData& flow, scalar rDeltaT, const dictionary& epsilonSolver, const dictionary& kSolver, scalar epsilonRelax,
                       scalar kRelax)
{
    const mi_ctx_t ctx = miEngine::New().ctx;
    const label n = k_.size();
    // volScalarField G(GName(), nut_*2*magSqr(symm(fvc::grad(U_))))  (:238)
    scalargpuField G(n);
    const double* grad[9];
    for (int j = 0; j < 3; ++j) for (int d = 0; d < 3; ++d) grad[3 * j + d] = flow.gradU[j]->component(d).data();
    miCheck(mi_ke_production(ctx, n, nut_.data(), grad, G.data()), "kEpsilon::correct: G");
    // epsilon_.boundaryField().updateCoeffs()  (:241)
    const scalargpuField epsilonOld(epsilon_), kOld(k_);
    mi_ke_wall w{};
    w.k_dev = k_.data(); w.b_delta_coeffs_dev = mesh_.bDeltaCoeffs->data(); w.b_y_dev = mesh_.y->data(); w.b_nuw_dev = bnu_.data();
    w.b_nutw_dev = bnut_.data(); w.g_inout_dev = G.data(); w.eps_inout_dev = epsilon_.data(); w.b_eps_out_dev = bepsilon_.data();
    for (int d = 0; d < 3; ++d) { w.u_dev[d] = flow.U->component(d).data(); w.b_uw_dev[d] = flow.bU->component(d).data(); }
    miCheck(mi_ke_wall_cells(h_, &coeffs_, &w), "epsilonWallFunction::updateCoeffs");
    // the dissipation equation (:244-258)
    scalargpuField su(n), sp(n), gamma(n);
    miCheck(mi_ke_epsilon_terms(ctx, n, &coeffs_, G.data(), epsilon_.data(), k_.data(), nut_.data(), nullptr, nu_, su.data(), sp.data(), gamma.data()),
            "kEpsilon::correct: epsEqn");
    solveEquation("epsilon", epsilon_, bepsilon_, epsilonOld, su, sp, gamma, coeffs_.sigmaEps, flow, rDeltaT, epsilonRelax, true, epsilonSolver);
    evaluateBoundary(epsilon_, bepsilon_);
    bound(epsilon_, &bepsilon_, *mesh_.average, *mesh_.weights, epsilonMin_);
    // the turbulent kinetic energy equation (:262-274)
    miCheck(mi_ke_k_terms(ctx, n, epsilon_.data(), k_.data(), nut_.data(), nullptr, nu_, sp.data(), gamma.data()), "kEpsilon::correct: kEqn");
    solveEquation("k", k_, bk_, kOld, G, sp, gamma, 1.0, flow, rDeltaT, kRelax, false, kSolver);
    evaluateBoundary(k_, bk_);
    bound(k_, &bk_, *mesh_.average, *mesh_.weights, kMin_);
    correctNut();                                           // :278-279
}

// ---- incompressible::RASModels::kOmegaSST -----------------------------------------------------------------------------------------------
kOmegaSST::kOmegaSST(const meshData& mesh, const flowData& flow, scalar nu, const scalargpuField& k, const scalargpuField& bk, const scalargpuField& omega,
                     const scalargpuField& bomega, const dictionary& coeffDict, scalar kMin, scalar omegaMin)
    : mesh_(mesh), nu_(nu), kMin_(kMin), omegaMin_(omegaMin), F3_(false), h_(nullptr), nb_(bk.size()), k_(k), omega_(omega), nut_(k.size()), bk_(bk),
      bomega_(bomega), bnut_(bk.size()), bnu_(std::vector<scalar>((std::size_t)bk.size(), nu)), F1_(k.size()), F23_(k.size()),
      ones_(std::vector<scalar>((std::size_t)k.size(), 1.0)), bOnes_(std::vector<scalar>((std::size_t)bk.size(), 1.0))
{
    const char* who = "kOmegaSST::New";
    if (!mesh.addr || !mesh.boundary || !mesh.average || !mesh.y || !mesh.bY || !mesh.Sf || !mesh.bSf)
        FatalErrorIn(who, "the addressing, the boundary, the averageData, the wall distance and the face area vectors are needed");
    if (mesh.patchTypes.size() != mesh.patchFaceCells.size()) FatalErrorIn(who, "one type per patch");
    // kOmegaSST.C:127-243 and the omega wall function's Cmu, kappa, E, beta1 (:406-409)
    const char* names[12] = {"alphaK1", "alphaK2", "alphaOmega1", "alphaOmega2", "gamma1", "gamma2", "beta1", "beta2", "betaStar", "a1", "b1", "c1"};
    mi_sst_coeffs d{};
    miCheck(mi_sst_coeffs_init(nullptr, nullptr, &d), who);
    scalar model[12] = {d.alphaK1, d.alphaK2, d.alphaOmega1, d.alphaOmega2, d.gamma1, d.gamma2, d.beta1, d.beta2, d.betaStar, d.a1, d.b1, d.c1};
    for (int i = 0; i < 12; ++i) coeffDict.readIfPresent(names[i], model[i]);
    scalar wall[4] = {d.Cmu, d.kappa, d.E, d.wallBeta1};
    coeffDict.readIfPresent("Cmu", wall[0]); coeffDict.readIfPresent("kappa", wall[1]); coeffDict.readIfPresent("E", wall[2]);
    coeffDict.readIfPresent("wallBeta1", wall[3]);
    scalar f3 = 0;
    coeffDict.readIfPresent("F3", f3);
    F3_ = f3 != 0;
    miCheck(mi_sst_coeffs_init(model, wall, &coeffs_), who);
    miCheck(mi_ke_coeffs_init(coeffs_.Cmu, 1.44, 1.92, 1.3, coeffs_.kappa, coeffs_.E, &wallCoeffs_), who);   // nutkWallFunction reads Cmu25, kappa, E, yPlusLam
    std::vector<int32_t> isWall;
    label off = 0;
    for (std::size_t p = 0; p < mesh.patchFaceCells.size(); ++p) {
        isWall.push_back(mesh.patchTypes[p] == wallFunction ? 1 : 0);
        start_.push_back(off);
        patches_.emplace_back(new fvPatchCells(mesh.addr->size(), mesh.patchFaceCells[p]));
        off += (label)mesh.patchFaceCells[p].size();
    }
    start_.push_back(off);
    if (off != nb_ || bomega.size() != nb_ || mesh.bY->size() != nb_) FatalErrorIn(who, "the boundary fields do not have one value per boundary face");
    miCheck(mi_ke_create(mesh.addr->handle(), mesh.boundary->handle(), isWall.data(), &h_), who);
    int32_t nWall = 0; const int32_t* labels = nullptr;
    miCheck(mi_ke_wall_cell_labels(h_, &nWall, &labels), who);
    labelgpuList cells(nWall);
    if (nWall) miCopyD2D(cells.data(), labels, sizeof(label) * (std::size_t)nWall);
    wallCells_.swap(cells);
    bound(k_, &bk_, *mesh_.average, *mesh_.weights, kMin_);             // :284
    bound(omega_, &bomega_, *mesh_.average, *mesh_.weights, omegaMin_); // :285
    // nut_ = a1_*k_/max(a1_*omega_, b1_*F23()*sqrt(2.0)*mag(symm(fvc::grad(U_)))); nut_.correctBoundaryConditions()  (:287-296)
    scalargpuField S2(k_.size()), G(k_.size()), mag(k_.size()), bS2(nb_), bG(nb_), bmag(nb_);
    production(S2, G, &mag, ones_, flow.gradU);
    production(bS2, bG, &bmag, bOnes_, flow.bGradU);
    correctNut(mag, bmag, true);
}
kOmegaSST::~kOmegaSST() { if (h_) mi_ke_destroy(h_); }
void kOmegaSST::production(scalargpuField& S2, scalargpuField& G, scalargpuField* mag, const scalargpuField& nut, const vectorgpuField* const* gradU) const
{
    const double* g[9];
    for (int j = 0; j < 3; ++j) for (int d = 0; d < 3; ++d) g[3 * j + d] = gradU[j]->component(d).data();
    miCheck(mi_sst_production(miEngine::New().ctx, nut.size(), nut.data(), g, S2.data(), G.data(), mag ? mag->data() : nullptr), "kOmegaSST: S2, G");
}
void kOmegaSST::correctNut(const scalargpuField& s, const scalargpuField& bs, bool constructorForm)
{
    const mi_ctx_t ctx = miEngine::New().ctx;
    miCheck(mi_sst_nut(ctx, k_.size(), &coeffs_, F3_, constructorForm, k_.data(), omega_.data(), mesh_.y->data(), s.data(), nullptr, nu_, nut_.data(),
                       nullptr), "kOmegaSST: nut");
    miCheck(mi_sst_nut(ctx, nb_, &coeffs_, F3_, constructorForm, bk_.data(), bomega_.data(), mesh_.bY->data(), bs.data(), nullptr, nu_, bnut_.data(),
                       nullptr), "kOmegaSST: nut");
    miCheck(mi_ke_nut_wall(h_, &wallCoeffs_, k_.data(), mesh_.bY->data(), bnu_.data(), bnut_.data(), nullptr), "nutkWallFunction::calcNut");
}
void kOmegaSST::evaluateBoundary(const scalargpuField& vf, scalargpuField& bvf) const
{
    for (std::size_t p = 0; p < patches_.size(); ++p)
        if (mesh_.patchTypes[p] != fixedValue && patches_[p]->size() > 0)
            miCheck(mi_patch_internal_field(patches_[p]->handle(), vf.data(), bvf.data() + start_[p]), "fvPatchField::evaluate");
}
void kOmegaSST::grad(vectorgpuField& g, vectorgpuField& bg, const scalargpuField& vf, const scalargpuField& bvf) const
{
    const mi_ctx_t ctx = miEngine::New().ctx;
    const lduAddressing& a = *mesh_.addr;
    const label n = a.size();
    scalargpuField ssf(mesh_.magSf->size());
    miCheck(mi_face_interpolate(a.handle(), mesh_.weights->data(), vf.data(), ssf.data()), "linear::interpolate");
    miCheck(mi_gauss_grad(a.handle(), mesh_.Sf->component(0).data(), mesh_.Sf->component(1).data(), mesh_.Sf->component(2).data(), ssf.data(), nullptr,
                          g.component(0).data(), g.component(1).data(), g.component(2).data()), "gaussGrad::gradf");
    for (std::size_t p = 0; p < patches_.size(); ++p) {
        if (patches_[p]->size() == 0) continue;
        for (direction d = 0; d < 3; ++d)
            miCheck(mi_patch_add_product(patches_[p]->handle(), mesh_.bSf->component(d).data() + start_[p], bvf.data() + start_[p], g.component(d).data(), 0),
                    "gaussGrad::gradf (patch)");
    }
    for (direction d = 0; d < 3; ++d) miCheck(mi_vec_div(ctx, n, g.component(d).data(), mesh_.V->data(), g.component(d).data()), "gaussGrad /= V");
    // gaussGrad::correctBoundaryConditions: snGrad = deltaCoeffs*(value - cell value) on every patch (zero where the value is the cell's)
    scalargpuField pif(nb_), diff(nb_), sn(std::vector<scalar>((std::size_t)nb_, 0.0));
    for (std::size_t p = 0; p < patches_.size(); ++p)
        if (patches_[p]->size() > 0) miCheck(mi_patch_internal_field(patches_[p]->handle(), vf.data(), pif.data() + start_[p]), "patchInternalField");
    fieldAxpby(diff, 1.0, bvf, -1.0, pif);
    fieldSubMul(sn, *mesh_.bDeltaCoeffs, diff);            // 0 - dc*diff, then the exact negation
    fieldAxpby(sn, -1.0, sn, 0.0, sn);
    for (std::size_t p = 0; p < patches_.size(); ++p) {
        if (patches_[p]->size() == 0) continue;
        const label s = start_[p];
        const double* snp[1] = {sn.data() + s};
        const double* gc[3] = {g.component(0).data(), g.component(1).data(), g.component(2).data()};
        double* out[3] = {bg.component(0).data() + s, bg.component(1).data() + s, bg.component(2).data() + s};
        miCheck(mi_patch_gauss_grad_correct(patches_[p]->handle(), 1, mesh_.bSf->component(0).data() + s, mesh_.bSf->component(1).data() + s,
                                            mesh_.bSf->component(2).data() + s, mesh_.bMagSf->data() + s, snp, gc, out), "gaussGrad::correctBoundaryConditions");
    }
}
void kOmegaSST::F23(scalargpuField& out) const
{
    scalargpuField nut(k_.size());
    miCheck(mi_sst_nut(miEngine::New().ctx, k_.size(), &coeffs_, F3_, 0, k_.data(), omega_.data(), mesh_.y->data(), ones_.data(), nullptr, nu_, nut.data(),
                       out.data()), "kOmegaSST::F23");
}
void kOmegaSST::F2(scalargpuField& out) const
{
    scalargpuField nut(k_.size());
    miCheck(mi_sst_nut(miEngine::New().ctx, k_.size(), &coeffs_, 0, 0, k_.data(), omega_.data(), mesh_.y->data(), ones_.data(), nullptr, nu_, nut.data(),
                       out.data()), "kOmegaSST::F2");
}
void kOmegaSST::F3(scalargpuField& out) const
{
    // 1 - tanh(pow4(arg3)): the optional output of the blending pass, which reads no gradient for it
    const label n = k_.size();
    scalargpuField zero(std::vector<scalar>((std::size_t)n, 0.0)), t[6] = {scalargpuField(n), scalargpuField(n), scalargpuField(n), scalargpuField(n),
                                                                            scalargpuField(n), scalargpuField(n)}, t3(n);
    mi_sst_blend_arrays x{};
    for (int d = 0; d < 3; ++d) { x.grad_k_dev[d] = zero.data(); x.grad_omega_dev[d] = zero.data(); }
    x.k_dev = k_.data(); x.omega_dev = omega_.data(); x.y_dev = mesh_.y->data(); x.nut_dev = nut_.data(); x.s2_dev = ones_.data(); x.nu_value = nu_;
    x.f1_out_dev = t[0].data(); x.su_out_dev = t[1].data(); x.sp_out_dev = t[2].data(); x.susp_out_dev = t[3].data(); x.domega_out_dev = t[4].data();
    x.dk_out_dev = t[5].data(); x.tanh3_out_dev_or_null = t3.data();
    miCheck(mi_sst_blend(miEngine::New().ctx, n, &coeffs_, 1, &x), "kOmegaSST::F3");
    fieldAxpby(out, 1.0, ones_, -1.0, t3);
}
void kOmegaSST::blend(scalargpuField& out, const scalargpuField& F1, scalar psi1, scalar psi2) const
{
#pragma clang fp contract(off)
    const scalar d = psi1 - psi2;
    fieldAxpby(out, d, F1, psi2, F1.size() == nb_ && nb_ != k_.size() ? bOnes_ : ones_);   // F1*(psi1 - psi2) + psi2: psi2*1 is exact
}
void kOmegaSST::DkEff(scalargpuField& out, const scalargpuField& F1) const
{
    const bool onBoundary = F1.size() == nb_ && nb_ != k_.size();
    scalargpuField a(F1.size()), m(std::vector<scalar>((std::size_t)F1.size(), 0.0));
    alphaK(a, F1);
    fieldSubMul(m, a, onBoundary ? bnut_ : nut_);          // 0 - alphaK*nut
    fieldAxpby(out, -1.0, m, nu_, onBoundary ? bOnes_ : ones_);
}
void kOmegaSST::DomegaEff(scalargpuField& out, const scalargpuField& F1) const
{
    const bool onBoundary = F1.size() == nb_ && nb_ != k_.size();
    scalargpuField a(F1.size()), m(std::vector<scalar>((std::size_t)F1.size(), 0.0));
    alphaOmega(a, F1);
    fieldSubMul(m, a, onBoundary ? bnut_ : nut_);
    fieldAxpby(out, -1.0, m, nu_, onBoundary ? bOnes_ : ones_);
}
solverPerformance kOmegaSST::solveEquation(const word& name, scalargpuField& psi, const scalargpuField& bpsi, const scalargpuField& psiOld,
                                           const scalargpuField& su, const scalargpuField& sp, const scalargpuField* susp, const scalargpuField& gamma,
                                           const scalargpuField& bGamma, const flowData& flow, scalar rDeltaT, scalar alpha, const dictionary& solverControls)
{
#pragma clang fp contract(off)
    const lduAddressing& a = *mesh_.addr;
    const label nf = mesh_.magSf->size();
    scalargpuField f(nf), gammaMagSf(std::vector<scalar>((std::size_t)nf, 0.0));
    fvc::interpolate(f, a, *mesh_.weights, gamma);
    fieldSubMul(gammaMagSf, f, *mesh_.magSf);               // 0 - f*magSf, then the exact negation
    fieldAxpby(gammaMagSf, -1.0, gammaMagSf, 0.0, gammaMagSf);
    std::vector<bool> coupled(mesh_.patchFaceCells.size(), false);
    fvScalarMatrix M(name, a, mesh_.patchFaceCells, coupled);
    mi_fvm_terms t{};
    const double* po[1] = {psiOld.data()}; const double* sd[1] = {su.data()}; const double sg[1] = {-1.0}; double* so[1] = {M.source().data()};
    t.ddt = 1; t.r_delta_t = rDeltaT; t.rho_value = 1.0; t.vol_dev = mesh_.V->data();
    t.div_flux_dev = flow.phi->data(); t.div_weights_dev = (flow.divWeights ? flow.divWeights : mesh_.weights)->data();
    t.lap_delta_coeffs_dev = mesh_.deltaCoeffs->data(); t.lap_gamma_magsf_dev = gammaMagSf.data();
    t.n_rhs = 1; t.psi_old_dev = po;
    if (!susp) {                                            // == su - fvm::Sp(sp, psi): one implicit part, inside the assembly
        t.sp_dev = sp.data(); t.sp_sign = 1.0;
        t.n_su = 1; t.su_dev = sd; t.su_sign = sg;
    }
    miCheck(mi_fvm_assemble(a.handle(), &t, M.lower().data(), M.upper().data(), M.diag().data(), so, nullptr), "kOmegaSST: fvm::assemble");
    if (susp)                                               // == su - fvm::Sp(sp, psi) - fvm::SuSp(susp, psi): the reference's grouping
        miCheck(mi_sst_omega_sources(miEngine::New().ctx, psi.size(), mesh_.V->data(), su.data(), sp.data(), susp->data(), psi.data(), M.diag().data(),
                                     M.source().data()), "kOmegaSST: omegaEqn sources");
    const std::vector<scalar> bg = bGamma.asHost(), bms = mesh_.bMagSf->asHost(), bdc = mesh_.bDeltaCoeffs->asHost(), bphi = flow.bPhi->asHost(),
                              bval = bpsi.asHost();
    for (std::size_t p = 0; p < patches_.size(); ++p) {
        const label m = start_[p + 1] - start_[p];
        std::vector<scalar> ic((std::size_t)m), bc((std::size_t)m);
        for (label i = 0; i < m; ++i) {
            const std::size_t j = (std::size_t)(start_[p] + i);
            if (mesh_.patchTypes[p] == fixedValue) {
                const scalar gm = bg[j] * bms[j], diff = gm * bdc[j];
                const scalar x = diff * bval[j], y = bphi[j] * bval[j];
                ic[(std::size_t)i] = diff; bc[(std::size_t)i] = x - y;
            } else { ic[(std::size_t)i] = bphi[j]; bc[(std::size_t)i] = 0.0; }
        }
        M.internalCoeffs()[p] = ic; M.boundaryCoeffs()[p] = bc;
    }
    M.relax(alpha, psi);
    if (susp && wallCells_.size() > 0) {                    // boundaryManipulate: omegaWallFunction::manipulateMatrix
        scalargpuField values(wallCells_.size());
        miCheck(mi_ke_wall_values(h_, psi.data(), values.data()), "omegaWallFunction::manipulateMatrix");
        M.setValues(wallCells_, values, psi);
    }
    return M.solve(psi, solverControls);
}
void kOmegaSST::correct(const flowData& flow, scalar rDeltaT, const dictionary& omegaSolver, const dictionary& kSolver, scalar omegaRelax, scalar kRelax)
{
    const mi_ctx_t ctx = miEngine::New().ctx;
    const label n = k_.size();
    // const volScalarField S2(2*magSqr(symm(fvc::grad(U_)))); volScalarField G(GName(), nut_*S2)  (:412-413)
    scalargpuField S2(n), G(n), bS2(nb_), bG(nb_);
    production(S2, G, nullptr, nut_, flow.gradU);
    production(bS2, bG, nullptr, bnut_, flow.bGradU);
    // omega_.boundaryField().updateCoeffs()  (:416)
    const scalargpuField omegaOld(omega_), kOld(k_);
    mi_sst_wall w{};
    w.k_dev = k_.data(); w.b_delta_coeffs_dev = mesh_.bDeltaCoeffs->data(); w.b_y_dev = mesh_.bY->data(); w.b_nuw_dev = bnu_.data();
    w.b_nutw_dev = bnut_.data(); w.g_inout_dev = G.data(); w.omega_inout_dev = omega_.data(); w.b_omega_out_dev = bomega_.data();
    for (int d = 0; d < 3; ++d) { w.u_dev[d] = flow.U->component(d).data(); w.b_uw_dev[d] = flow.bU->component(d).data(); }
    miCheck(mi_sst_wall_cells(h_, &coeffs_, &w), "omegaWallFunction::updateCoeffs");
    // CDkOmega, F1 and everything blended with it (:418-439), on the cells and on the boundary faces
    vectorgpuField gradK(n), gradOmega(n), bGradK(nb_), bGradOmega(nb_);
    grad(gradK, bGradK, k_, bk_);
    grad(gradOmega, bGradOmega, omega_, bomega_);
    scalargpuField su(n), sp(n), susp(n), DomegaEff(n), DkEff(n);
    scalargpuField bF1(nb_), bF23(nb_), bsu(nb_), bsp(nb_), bsusp(nb_), bDomegaEff(nb_), bDkEff(nb_);
    auto blendPass = [&](label m, const vectorgpuField& gk, const vectorgpuField& go, const scalargpuField& k, const scalargpuField& omega, const scalargpuField& y,
                         const scalargpuField& nut, const scalargpuField& s2, scalargpuField& F1, scalargpuField& F23, scalargpuField& a, scalargpuField& b,
                         scalargpuField& c, scalargpuField& dO, scalargpuField& dK) {
        mi_sst_blend_arrays x{};
        for (int d = 0; d < 3; ++d) { x.grad_k_dev[d] = gk.component(d).data(); x.grad_omega_dev[d] = go.component(d).data(); }
        x.k_dev = k.data(); x.omega_dev = omega.data(); x.y_dev = y.data(); x.nut_dev = nut.data(); x.s2_dev = s2.data(); x.nu_value = nu_;
        x.f1_out_dev = F1.data(); x.su_out_dev = a.data(); x.sp_out_dev = b.data(); x.susp_out_dev = c.data(); x.domega_out_dev = dO.data();
        x.dk_out_dev = dK.data(); x.f23_out_dev_or_null = F23.data();
        miCheck(mi_sst_blend(ctx, m, &coeffs_, F3_, &x), "kOmegaSST::correct: F1");
    };
    blendPass(n, gradK, gradOmega, k_, omega_, *mesh_.y, nut_, S2, F1_, F23_, su, sp, susp, DomegaEff, DkEff);
    blendPass(nb_, bGradK, bGradOmega, bk_, bomega_, *mesh_.bY, bnut_, bS2, bF1, bF23, bsu, bsp, bsusp, bDomegaEff, bDkEff);
    // the turbulent frequency equation (:426-447)
    solveEquation("omega", omega_, bomega_, omegaOld, su, sp, &susp, DomegaEff, bDomegaEff, flow, rDeltaT, omegaRelax, omegaSolver);
    evaluateBoundary(omega_, bomega_);
    bound(omega_, &bomega_, *mesh_.average, *mesh_.weights, omegaMin_);
    // the turbulent kinetic energy equation (:450-462)
    miCheck(mi_sst_k_terms(ctx, n, &coeffs_, G.data(), k_.data(), omega_.data(), su.data(), sp.data()), "kOmegaSST::correct: kEqn");
    solveEquation("k", k_, bk_, kOld, su, sp, nullptr, DkEff, bDkEff, flow, rDeltaT, kRelax, kSolver);
    evaluateBoundary(k_, bk_);
    bound(k_, &bk_, *mesh_.average, *mesh_.weights, kMin_);
    correctNut(S2, bS2, false);                             // :466-467
}
}
}
// ---- the Spalart-Allmaras model: RAS, DES, DDES, IDDES ---------------------------------------------------------------------
namespace incompressible
{
struct SpalartAllmarasBase::termFields
{
    scalargpuField suGrad, suProd, sp, dnu, fv1;
    scalargpuField *S, *dTilda, *tanhFd;                    // optional
    explicit termFields(label m) : suGrad(m), suProd(m), sp(m), dnu(m), fv1(m), S(nullptr), dTilda(nullptr), tanhFd(nullptr) {}
};
SpalartAllmarasBase::SpalartAllmarasBase(const meshData& mesh, scalar nu, const scalargpuField& nuTilda, const scalargpuField& bnuTilda,
                                         const dictionary& coeffDict)
    : mesh_(mesh), nu_(nu), ashfordCorrection_(true), h_(nullptr), nb_(bnuTilda.size()), nuTilda_(nuTilda), bnuTilda_(bnuTilda), nut_(nuTilda.size()),
      bnut_(std::vector<scalar>((std::size_t)bnuTilda.size(), 0.0)), bnu_(std::vector<scalar>((std::size_t)bnuTilda.size(), nu))
{
    const char* who = "SpalartAllmaras::New";
    if (!mesh.addr || !mesh.boundary || !mesh.average || !mesh.y || !mesh.bY || !mesh.Sf || !mesh.bSf)
        FatalErrorIn(who, "the addressing, the boundary, the averageData, the wall distance and the face area vectors are needed");
    if (mesh.patchTypes.size() != mesh.patchFaceCells.size()) FatalErrorIn(who, "one type per patch");
    const char* names[13] = {"sigmaNut", "kappa", "Cb1", "Cb2", "Cw2", "Cw3", "Cv1", "Cv2", "CDES", "ck", "fwStar", "cl", "ct"};
    mi_sa_coeffs d{};
    miCheck(mi_sa_coeffs_init(nullptr, nullptr, &d), who);
    scalar model[13] = {d.sigmaNut, d.kappa, d.Cb1, d.Cb2, d.Cw2, d.Cw3, d.Cv1, d.Cv2, d.CDES, d.ck, d.fwStar, d.cl, d.ct};
    for (int i = 0; i < 13; ++i) coeffDict.readIfPresent(names[i], model[i]);
    scalar wall[2] = {d.wallKappa, d.E};                    // the wall function's own kappa and E
    coeffDict.readIfPresent("wallKappa", wall[0]); coeffDict.readIfPresent("E", wall[1]);
    scalar ash = 1;
    coeffDict.readIfPresent("ashfordCorrection", ash);
    ashfordCorrection_ = ash != 0;
    miCheck(mi_sa_coeffs_init(model, wall, &coeffs_), who);
    sigmaNut_ = coeffs_.sigmaNut; kappa_ = coeffs_.kappa; Cb1_ = coeffs_.Cb1; Cb2_ = coeffs_.Cb2; Cw1_ = coeffs_.Cw1; Cw2_ = coeffs_.Cw2; Cw3_ = coeffs_.Cw3;
    Cv1_ = coeffs_.Cv1; Cv2_ = coeffs_.Cv2; CDES_ = coeffs_.CDES; ck_ = coeffs_.ck; fwStar_ = coeffs_.fwStar; cl_ = coeffs_.cl; ct_ = coeffs_.ct;
    std::vector<int32_t> isWall;
    label off = 0;
    for (std::size_t p = 0; p < mesh.patchFaceCells.size(); ++p) {
        isWall.push_back(mesh.patchTypes[p] == wallFunction ? 1 : 0);
        start_.push_back(off);
        patches_.emplace_back(new fvPatchCells(mesh.addr->size(), mesh.patchFaceCells[p]));
        off += (label)mesh.patchFaceCells[p].size();
    }
    start_.push_back(off);
    if (off != nb_ || mesh.bY->size() != nb_) FatalErrorIn(who, "the boundary fields do not have one value per boundary face");
    miCheck(mi_ke_create(mesh.addr->handle(), mesh.boundary->handle(), isWall.data(), &h_), who);
}
SpalartAllmarasBase::~SpalartAllmarasBase() { if (h_) mi_ke_destroy(h_); }
void SpalartAllmarasBase::evaluateBoundary(const scalargpuField& vf, scalargpuField& bvf) const
{
    for (std::size_t p = 0; p < patches_.size(); ++p)
        if (mesh_.patchTypes[p] != fixedValue && patches_[p]->size() > 0)
            miCheck(mi_patch_internal_field(patches_[p]->handle(), vf.data(), bvf.data() + start_[p]), "fvPatchField::evaluate");
}
void SpalartAllmarasBase::grad(vectorgpuField& g, vectorgpuField& bg, const scalargpuField& vf, const scalargpuField& bvf) const
{
    // kOmegaSST::grad: fvc::grad with `Gauss linear` and gaussGrad::correctBoundaryConditions
    const mi_ctx_t ctx = miEngine::New().ctx;
    const lduAddressing& a = *mesh_.addr;
    const label n = a.size();
    scalargpuField ssf(mesh_.magSf->size());
    miCheck(mi_face_interpolate(a.handle(), mesh_.weights->data(), vf.data(), ssf.data()), "linear::interpolate");
    miCheck(mi_gauss_grad(a.handle(), mesh_.Sf->component(0).data(), mesh_.Sf->component(1).data(), mesh_.Sf->component(2).data(), ssf.data(), nullptr,
                          g.component(0).data(), g.component(1).data(), g.component(2).data()), "gaussGrad::gradf");
    for (std::size_t p = 0; p < patches_.size(); ++p) {
        if (patches_[p]->size() == 0) continue;
        for (direction d = 0; d < 3; ++d)
            miCheck(mi_patch_add_product(patches_[p]->handle(), mesh_.bSf->component(d).data() + start_[p], bvf.data() + start_[p], g.component(d).data(), 0),
                    "gaussGrad::gradf (patch)");
    }
    for (direction d = 0; d < 3; ++d) miCheck(mi_vec_div(ctx, n, g.component(d).data(), mesh_.V->data(), g.component(d).data()), "gaussGrad /= V");
    scalargpuField pif(nb_), diff(nb_), sn(std::vector<scalar>((std::size_t)nb_, 0.0));
    for (std::size_t p = 0; p < patches_.size(); ++p)
        if (patches_[p]->size() > 0) miCheck(mi_patch_internal_field(patches_[p]->handle(), vf.data(), pif.data() + start_[p]), "patchInternalField");
    fieldAxpby(diff, 1.0, bvf, -1.0, pif);
    fieldSubMul(sn, *mesh_.bDeltaCoeffs, diff);            // 0 - dc*diff, then the exact negation
    fieldAxpby(sn, -1.0, sn, 0.0, sn);
    for (std::size_t p = 0; p < patches_.size(); ++p) {
        if (patches_[p]->size() == 0) continue;
        const label s = start_[p];
        const double* snp[1] = {sn.data() + s};
        const double* gc[3] = {g.component(0).data(), g.component(1).data(), g.component(2).data()};
        double* out[3] = {bg.component(0).data() + s, bg.component(1).data() + s, bg.component(2).data() + s};
        miCheck(mi_patch_gauss_grad_correct(patches_[p]->handle(), 1, mesh_.bSf->component(0).data() + s, mesh_.bSf->component(1).data() + s,
                                            mesh_.bSf->component(2).data() + s, mesh_.bMagSf->data() + s, snp, gc, out), "gaussGrad::correctBoundaryConditions");
    }
}
void SpalartAllmarasBase::terms(int kind, bool onBoundary, const flowData& flow, const vectorgpuField& gradNuTilda, termFields& o) const
{
    const char* who = "SpalartAllmaras: mi_sa_terms";
    if (kind >= MI_SA_DES && (!mesh_.delta || !mesh_.bDelta)) FatalErrorIn(who, "the DES kinds need meshData::delta and bDelta");
    if (kind == MI_SA_IDDES && (!mesh_.hmax || !mesh_.bHmax)) FatalErrorIn(who, "IDDES needs meshData::hmax and bHmax");
    const vectorgpuField* const* g = onBoundary ? flow.bGradU : flow.gradU;
    mi_sa_cells x{};
    x.nutilda_dev = (onBoundary ? bnuTilda_ : nuTilda_).data();
    for (int j = 0; j < 3; ++j) for (int d = 0; d < 3; ++d) x.grad_dev[3 * j + d] = g[j]->component(d).data();
    for (int d = 0; d < 3; ++d) x.grad_nutilda_dev[d] = gradNuTilda.component(d).data();
    x.y_dev = (onBoundary ? mesh_.bY : mesh_.y)->data();
    x.nu_value = nu_;
    if (kind >= MI_SA_DES) x.delta_dev = (onBoundary ? mesh_.bDelta : mesh_.delta)->data();
    if (kind >= MI_SA_DDES) x.nusgs_dev = (onBoundary ? bnut_ : nut_).data();
    if (kind == MI_SA_IDDES) x.hmax_dev = (onBoundary ? mesh_.bHmax : mesh_.hmax)->data();
    x.su_grad_out_dev = o.suGrad.data(); x.su_prod_out_dev = o.suProd.data(); x.sp_out_dev = o.sp.data(); x.dnu_out_dev = o.dnu.data();
    x.fv1_out_dev = o.fv1.data();
    if (o.S) x.s_out_dev_or_null = o.S->data();
    if (o.dTilda) x.dtilda_out_dev_or_null = o.dTilda->data();
    if (o.tanhFd) x.tanh_fd_out_dev_or_null = o.tanhFd->data();
    miCheck(mi_sa_terms(miEngine::New().ctx, o.sp.size(), &coeffs_, kind, ashfordCorrection_ ? 1 : 0, &x), who);
}
void SpalartAllmarasBase::field(int kind, int which, scalargpuField& out, const flowData& flow) const
{
    const label n = nuTilda_.size();
    vectorgpuField g(n), bg(nb_);
    grad(g, bg, nuTilda_, bnuTilda_);
    termFields o(n);
    scalargpuField t(n);
    if (which == 0) o.S = &out; else if (which == 1) o.dTilda = &out; else o.tanhFd = &t;
    terms(kind, false, flow, g, o);
    if (which == 2) {                                       // fd = 1 - tanh(...)
        const scalargpuField ones(std::vector<scalar>((std::size_t)n, 1.0));
        fieldAxpby(out, 1.0, ones, -1.0, t);
    }
}
void SpalartAllmarasBase::DnuTildaEff(scalargpuField& out) const
{
    const scalargpuField nuField(std::vector<scalar>((std::size_t)nuTilda_.size(), nu_));
    scalargpuField sum(nuTilda_.size());
    fieldAxpby(sum, 1.0, nuTilda_, 1.0, nuField);
    const scalargpuField sig(std::vector<scalar>((std::size_t)nuTilda_.size(), sigmaNut_));
    miCheck(mi_vec_div(miEngine::New().ctx, sum.size(), sum.data(), sig.data(), out.data()), "SpalartAllmaras::DnuTildaEff");
}
void SpalartAllmarasBase::correctNut(const flowData& flow, const scalargpuField* fv1, const scalargpuField* bfv1)
{
    const mi_ctx_t ctx = miEngine::New().ctx;
    const char* who = "SpalartAllmaras: nut";
    scalargpuField bcalc(nb_);
    miCheck(mi_sa_nut(ctx, nuTilda_.size(), &coeffs_, fv1 ? 0 : 1, nuTilda_.data(), fv1 ? fv1->data() : nullptr, nullptr, nu_, nut_.data(), nullptr), who);
    miCheck(mi_sa_nut(ctx, nb_, &coeffs_, bfv1 ? 0 : 1, bnuTilda_.data(), bfv1 ? bfv1->data() : nullptr, nullptr, nu_, bcalc.data(), nullptr), who);
    // a calculated patch takes the formula on its boundary values; a nutUSpaldingWallFunction patch keeps its value, which calcNut reads
    for (std::size_t p = 0; p < patches_.size(); ++p)
        if (mesh_.patchTypes[p] != wallFunction && patches_[p]->size() > 0)
            miCopyD2D(bnut_.data() + start_[p], bcalc.data() + start_[p], sizeof(scalar) * (std::size_t)(start_[p + 1] - start_[p]));
    mi_sa_wall w{};
    for (int d = 0; d < 3; ++d) { w.u_dev[d] = flow.U->component(d).data(); w.b_uw_dev[d] = flow.bU->component(d).data(); }
    w.b_delta_coeffs_dev = mesh_.bDeltaCoeffs->data(); w.b_y_dev = mesh_.bY->data(); w.b_nuw_dev = bnu_.data(); w.b_nutw_inout_dev = bnut_.data();
    miCheck(mi_sa_nut_spalding_wall(h_, &coeffs_, &w), "nutUSpaldingWallFunction::calcNut");
}
void SpalartAllmarasBase::correct(const flowData& flow, scalar rDeltaT, const dictionary& solverControls, scalar alpha)
{
#pragma clang fp contract(off)
    const lduAddressing& a = *mesh_.addr;
    const label n = nuTilda_.size(), nf = mesh_.magSf->size();
    vectorgpuField gradNuTilda(n), bGradNuTilda(nb_);
    grad(gradNuTilda, bGradNuTilda, nuTilda_, bnuTilda_);
    termFields o(n), b(nb_);
    terms(kind(), false, flow, gradNuTilda, o);
    terms(kind(), true, flow, bGradNuTilda, b);
    // fvm::ddt(nuTilda) + fvm::div(phi, nuTilda) - fvm::laplacian(DnuTildaEff, nuTilda) - Cb2/sigmaNut*magSqr(grad(nuTilda))
    //  == Cb1*STilda*nuTilda - fvm::Sp(Cw1*fw*nuTilda/sqr(dTilda), nuTilda)   (RAS :446-455, LES :335-349)
    const scalargpuField nuTildaOld(nuTilda_);
    scalargpuField f(nf), gammaMagSf(std::vector<scalar>((std::size_t)nf, 0.0));
    fvc::interpolate(f, a, *mesh_.weights, o.dnu);
    fieldSubMul(gammaMagSf, f, *mesh_.magSf);               // 0 - f*magSf, then the exact negation
    fieldAxpby(gammaMagSf, -1.0, gammaMagSf, 0.0, gammaMagSf);
    std::vector<bool> coupled(mesh_.patchFaceCells.size(), false);
    fvScalarMatrix M("nuTilda", a, mesh_.patchFaceCells, coupled);
    mi_fvm_terms t{};
    const double* po[1] = {nuTildaOld.data()}; const double* sd[2] = {o.suGrad.data(), o.suProd.data()}; const double sg[2] = {-1.0, -1.0};
    double* so[1] = {M.source().data()};
    t.ddt = 1; t.r_delta_t = rDeltaT; t.rho_value = 1.0; t.vol_dev = mesh_.V->data();
    t.div_flux_dev = flow.phi->data(); t.div_weights_dev = (flow.divWeights ? flow.divWeights : mesh_.weights)->data();
    t.lap_delta_coeffs_dev = mesh_.deltaCoeffs->data(); t.lap_gamma_magsf_dev = gammaMagSf.data();
    t.n_rhs = 1; t.psi_old_dev = po;
    t.sp_dev = o.sp.data(); t.sp_sign = 1.0;
    t.n_su = 2; t.su_dev = sd; t.su_sign = sg;              // (source + V*su_grad) + V*su_prod, the reference's grouping
    miCheck(mi_fvm_assemble(a.handle(), &t, M.lower().data(), M.upper().data(), M.diag().data(), so, nullptr), "SpalartAllmaras: fvm::assemble");
    const std::vector<scalar> bg = b.dnu.asHost(), bms = mesh_.bMagSf->asHost(), bdc = mesh_.bDeltaCoeffs->asHost(), bphi = flow.bPhi->asHost(),
                              bval = bnuTilda_.asHost();
    for (std::size_t p = 0; p < patches_.size(); ++p) {
        const label m = start_[p + 1] - start_[p];
        std::vector<scalar> ic((std::size_t)m), bc((std::size_t)m);
        for (label i = 0; i < m; ++i) {
            const std::size_t j = (std::size_t)(start_[p] + i);
            if (mesh_.patchTypes[p] == fixedValue) {
                const scalar gm = bg[j] * bms[j], diff = gm * bdc[j];
                const scalar x = diff * bval[j], y = bphi[j] * bval[j];
                ic[(std::size_t)i] = diff; bc[(std::size_t)i] = x - y;
            } else { ic[(std::size_t)i] = bphi[j]; bc[(std::size_t)i] = 0.0; }
        }
        M.internalCoeffs()[p] = ic; M.boundaryCoeffs()[p] = bc;
    }
    M.relax(alpha, nuTilda_);
    M.solve(nuTilda_, solverControls);
    evaluateBoundary(nuTilda_, bnuTilda_);
    bound(nuTilda_, &bnuTilda_, *mesh_.average, *mesh_.weights, 0.0);
    if (storedFv1()) correctNut(flow, &o.fv1, &b.fv1); else correctNut(flow, nullptr, nullptr);
}
namespace RASModels
{
SpalartAllmaras::SpalartAllmaras(const meshData& mesh, const flowData& flow, scalar nu, const scalargpuField& nuTilda, const scalargpuField& bnuTilda,
                                 const dictionary& coeffDict)
    : SpalartAllmarasBase(mesh, nu, nuTilda, bnuTilda, coeffDict)
{
    correctNut(flow, nullptr, nullptr);                     // nut_ = nuTilda_*fv1(this->chi()) (:426): the reference reads nut; here it is formed
}
}
namespace LESModels
{
SpalartAllmaras::SpalartAllmaras(const meshData& mesh, scalar nu, const scalargpuField& nuTilda, const scalargpuField& bnuTilda, const dictionary& coeffDict, bool)
    : SpalartAllmarasBase(mesh, nu, nuTilda, bnuTilda, coeffDict) {}
SpalartAllmaras::SpalartAllmaras(const meshData& mesh, const flowData& flow, scalar nu, const scalargpuField& nuTilda, const scalargpuField& bnuTilda,
                                 const dictionary& coeffDict)
    : SpalartAllmarasBase(mesh, nu, nuTilda, bnuTilda, coeffDict)
{
    updateSubGridScaleFields(flow);                         // :310
}
void SpalartAllmaras::updateSubGridScaleFields(const flowData& flow) { correctNut(flow, nullptr, nullptr); }
void SpalartAllmaras::S(scalargpuField& out, const flowData& flow) const { field(MI_SA_DES, 0, out, flow); }
void SpalartAllmaras::dTilda(scalargpuField& out, const flowData& flow) const { field(MI_SA_DES, 1, out, flow); }
SpalartAllmarasDDES::SpalartAllmarasDDES(const meshData& mesh, const flowData& flow, scalar nu, const scalargpuField& nuTilda, const scalargpuField& bnuTilda,
                                         const dictionary& coeffDict)
    : SpalartAllmaras(mesh, nu, nuTilda, bnuTilda, coeffDict, true)
{
    updateSubGridScaleFields(flow);
}
void SpalartAllmarasDDES::fd(scalargpuField& out, const flowData& flow) const { field(MI_SA_DDES, 2, out, flow); }
void SpalartAllmarasDDES::S(scalargpuField& out, const flowData& flow) const { field(MI_SA_DDES, 0, out, flow); }
void SpalartAllmarasDDES::dTilda(scalargpuField& out, const flowData& flow) const { field(MI_SA_DDES, 1, out, flow); }
SpalartAllmarasIDDES::SpalartAllmarasIDDES(const meshData& mesh, const flowData& flow, scalar nu, const scalargpuField& nuTilda, const scalargpuField& bnuTilda,
                                           const dictionary& coeffDict)
    : SpalartAllmaras(mesh, nu, nuTilda, bnuTilda, coeffDict, true)
{
    updateSubGridScaleFields(flow);
}
void SpalartAllmarasIDDES::fd(scalargpuField& out, const flowData& flow) const { field(MI_SA_IDDES, 2, out, flow); }
void SpalartAllmarasIDDES::dTilda(scalargpuField& out, const flowData& flow) const { field(MI_SA_IDDES, 1, out, flow); }
}
}
// ---- LESdelta, simpleFilter and incompressible::LESModels -------------------------------------------------------------------
LESdelta::LESdelta(label nCells, label nBoundaryFaces)
    : delta_(std::vector<scalar>((std::size_t)nCells, 1e-15)), bdelta_(std::vector<scalar>((std::size_t)nBoundaryFaces, 1e-15)) {}   // LESdelta.C:53
LESdelta::~LESdelta() {}
cubeRootVolDelta::cubeRootVolDelta(const scalargpuField& V, label nBoundaryFaces, scalar deltaCoeff, scalar thickness)
    : LESdelta(V.size(), nBoundaryFaces), deltaCoeff_(deltaCoeff), thickness_(thickness)
{
    calcDelta(V);
}
void cubeRootVolDelta::calcDelta(const scalargpuField& V)
{
    miCheck(mi_les_delta_cube_root_vol(miEngine::New().ctx, V.size(), deltaCoeff_, thickness_, V.data(), delta_.data(), nullptr), "cubeRootVolDelta::calcDelta");
}
simpleFilter::simpleFilter(const averageData& av, const scalargpuField& weights) : av_(&av), weights_(&weights) {}
void simpleFilter::operator()(const std::vector<const scalargpuField*>& vf, const std::vector<const scalargpuField*>& bvf,
                              const std::vector<scalargpuField*>& out) const
{
    if (vf.empty() || vf.size() > 9 || out.size() != vf.size() || (!bvf.empty() && bvf.size() != vf.size()))
        FatalErrorIn("simpleFilter::operator()", "one to nine components, as many outputs and boundary fields");
    const double* v[9] = {}; const double* b[9] = {}; double* o[9] = {};
    for (std::size_t i = 0; i < vf.size(); ++i) { v[i] = vf[i]->data(); o[i] = out[i]->data(); if (!bvf.empty()) b[i] = bvf[i]->data(); }
    miCheck(mi_les_simple_filter(av_->handle(), (int)vf.size(), weights_->data(), av_->magSf().data(), av_->bMagSf() ? av_->bMagSf()->data() : nullptr,
                                 v, bvf.empty() ? nullptr : b, o), "simpleFilter::operator()");
}
namespace incompressible
{
namespace LESModels
{
namespace
{
std::vector<const scalargpuField*> cptrs(const std::vector<scalargpuField>& v, std::size_t a, std::size_t b)
{
    std::vector<const scalargpuField*> p;
    for (std::size_t i = a; i < b; ++i) p.push_back(&v[i]);
    return p;
}
std::vector<scalargpuField*> mptrs(std::vector<scalargpuField>& v, std::size_t a, std::size_t b)
{
    std::vector<scalargpuField*> p;
    for (std::size_t i = a; i < b; ++i) p.push_back(&v[i]);
    return p;
}
void dataOf(const std::vector<scalargpuField>& v, std::size_t a, const double** out, int n) { for (int i = 0; i < n; ++i) out[i] = v[a + (std::size_t)i].data(); }
void dataOf(std::vector<scalargpuField>& v, std::size_t a, double** out, int n) { for (int i = 0; i < n; ++i) out[i] = v[a + (std::size_t)i].data(); }
}
GenEddyVisc::GenEddyVisc(const meshData& mesh, scalar nu, const scalargpuField& k, const scalargpuField& bk, const dictionary& coeffDict, scalar kMin)
    : mesh_(mesh), nu_(nu), kMin_(kMin), nb_(bk.size()), delta_(*mesh.V, bk.size(), coeffDict.lookupOrDefault<scalar>("deltaCoeff", 1.0)), k_(k), bk_(bk),
      nuSgs_(k.size()), bnuSgs_(bk.size())
{
    const char* who = "GenEddyVisc::New";
    if (!mesh.addr || !mesh.boundary || !mesh.average) FatalErrorIn(who, "the addressing, the boundary and the averageData are needed");
    if (mesh.patchTypes.size() != mesh.patchFaceCells.size()) FatalErrorIn(who, "one type per patch");
    scalar ck = 0.094, ce = 1.048;
    coeffDict.readIfPresent("ck", ck); coeffDict.readIfPresent("ce", ce);
    miCheck(mi_les_coeffs_init(ck, ce, &coeffs_), who);
    label off = 0;
    for (std::size_t p = 0; p < mesh.patchFaceCells.size(); ++p) {
        start_.push_back(off);
        patches_.emplace_back(new fvPatchCells(mesh.addr->size(), mesh.patchFaceCells[p]));
        off += (label)mesh.patchFaceCells[p].size();
    }
    start_.push_back(off);
    if (off != nb_) FatalErrorIn(who, "the boundary fields do not have one value per boundary face");
}
GenEddyVisc::~GenEddyVisc() {}
void GenEddyVisc::evaluateBoundary(const scalargpuField& vf, scalargpuField& bvf, bool keepFixed) const
{
    for (std::size_t p = 0; p < patches_.size(); ++p)
        if (!(keepFixed && mesh_.patchTypes[p] == fixedValue) && patches_[p]->size() > 0)
            miCheck(mi_patch_internal_field(patches_[p]->handle(), vf.data(), bvf.data() + start_[p]), "fvPatchField::evaluate");
}
void GenEddyVisc::gradArrays(const vectorgpuField* const* g, const double* out[9])
{
    for (int j = 0; j < 3; ++j) for (int d = 0; d < 3; ++d) out[3 * j + d] = g[j]->component((direction)d).data();
}
void GenEddyVisc::nuEff(scalargpuField& out) const { DkEff(out); }
void GenEddyVisc::DkEff(scalargpuField& out) const
{
    scalargpuField sp(nuSgs_.size());                       // mi_ke_k_terms' dk = nut + nu; its sp is not used
    miCheck(mi_ke_k_terms(miEngine::New().ctx, nuSgs_.size(), k_.data(), k_.data(), nuSgs_.data(), nullptr, nu_, sp.data(), out.data()), "GenEddyVisc::DkEff");
}
void GenEddyVisc::divDevReff(fvVectorMatrix& UEqn, const vectorgpuField& Sf, const vectorgpuField* const gradU[3],
                             const std::vector<fvc::devTGradPatch>& patches) const
{
    scalargpuField visc(k_.size());
    nuEff(visc);
    vectorgpuField div(k_.size());
    fvc::divDevTGrad(div, *mesh_.addr, fvc::DEV, *mesh_.weights, Sf, visc, gradU, patches, *mesh_.V);
    UEqn.subtractField(div, *mesh_.V);
}
void GenEddyVisc::solveK(const scalargpuField& G, const scalargpuField& sp, const scalargpuField& gamma, const flowData& flow, scalar rDeltaT, scalar alpha,
                         const dictionary& solverControls)
{
#pragma clang fp contract(off)
    const lduAddressing& a = *mesh_.addr;
    const label nf = mesh_.magSf->size();
    const scalargpuField kOld(k_);
    scalargpuField f(nf), gammaMagSf(nf);
    fvc::interpolate(f, a, *mesh_.weights, gamma);
    fieldSubMul(gammaMagSf, f, *mesh_.magSf);               // 0 - f*magSf, then the exact negation
    fieldAxpby(gammaMagSf, -1.0, gammaMagSf, 0.0, gammaMagSf);
    std::vector<bool> coupled(mesh_.patchFaceCells.size(), false);
    fvScalarMatrix M("k", a, mesh_.patchFaceCells, coupled);
    mi_fvm_terms t{};
    const double* po[1] = {kOld.data()}; const double* sd[1] = {G.data()}; const double sg[1] = {-1.0}; double* so[1] = {M.source().data()};
    t.ddt = 1; t.r_delta_t = rDeltaT; t.rho_value = 1.0; t.vol_dev = mesh_.V->data();
    t.div_flux_dev = flow.phi->data(); t.div_weights_dev = (flow.divWeights ? flow.divWeights : mesh_.weights)->data();
    t.lap_delta_coeffs_dev = mesh_.deltaCoeffs->data(); t.lap_gamma_magsf_dev = gammaMagSf.data();
    t.sp_dev = sp.data(); t.sp_sign = 1.0;
    t.n_rhs = 1; t.psi_old_dev = po; t.n_su = 1; t.su_dev = sd; t.su_sign = sg;
    miCheck(mi_fvm_assemble(a.handle(), &t, M.lower().data(), M.upper().data(), M.diag().data(), so, nullptr), "GenEddyVisc: fvm::assemble");
    // fixedValue: the diffusion coefficient and (diff - phi)*value with the boundary DkEff = nuSgs_b + nu; zeroGradient: the flux and nothing
    const std::vector<scalar> bnut = bnuSgs_.asHost(), bms = mesh_.bMagSf->asHost(), bdc = mesh_.bDeltaCoeffs->asHost(), bphi = flow.bPhi->asHost(),
                              bval = bk_.asHost();
    for (std::size_t p = 0; p < patches_.size(); ++p) {
        const label m = start_[p + 1] - start_[p];
        std::vector<scalar> ic((std::size_t)m), bc((std::size_t)m);
        for (label i = 0; i < m; ++i) {
            const std::size_t j = (std::size_t)(start_[p] + i);
            if (mesh_.patchTypes[p] == fixedValue) {
                const scalar g = bnut[j] + nu_, gm = g * bms[j], diff = gm * bdc[j];
                const scalar x = diff * bval[j], y = bphi[j] * bval[j];
                ic[(std::size_t)i] = diff; bc[(std::size_t)i] = x - y;
            } else { ic[(std::size_t)i] = bphi[j]; bc[(std::size_t)i] = 0.0; }
        }
        M.internalCoeffs()[p] = ic; M.boundaryCoeffs()[p] = bc;
    }
    M.relax(alpha, k_);
    M.solve(k_, solverControls);
    evaluateBoundary(k_, bk_, true);
    bound(k_, &bk_, *mesh_.average, *mesh_.weights, kMin_);
}

Smagorinsky::Smagorinsky(const meshData& mesh, const flowData& flow, scalar nu, const dictionary& coeffDict)
    : GenEddyVisc(mesh, nu, scalargpuField(mesh.V->size()), scalargpuField(mesh.bMagSf->size()), coeffDict, 1e-15)
{
    updateSubGridScaleFields(flow);                         // Smagorinsky.C:76
}
void Smagorinsky::updateSubGridScaleFields(const flowData& flow)
{
    const double* grad[9];
    gradArrays(flow.gradU, grad);
    miCheck(mi_les_smagorinsky(miEngine::New().ctx, k_.size(), &coeffs_, delta_().data(), grad, k_.data(), nuSgs_.data()), "Smagorinsky::updateSubGridScaleFields");
    evaluateBoundary(nuSgs_, bnuSgs_, false);
    evaluateBoundary(k_, bk_, false);
}
void Smagorinsky::correct(const flowData& flow, scalar, const dictionary&, scalar) { updateSubGridScaleFields(flow); }   // Smagorinsky.C:84-89

oneEqEddy::oneEqEddy(const meshData& mesh, scalar nu, const scalargpuField& k, const scalargpuField& bk, const dictionary& coeffDict, scalar kMin)
    : GenEddyVisc(mesh, nu, k, bk, coeffDict, kMin)
{
    bound(k_, &bk_, *mesh_.average, *mesh_.weights, kMin_);   // oneEqEddy.C:90
    updateSubGridScaleFields();
}
void oneEqEddy::updateSubGridScaleFields()
{
    miCheck(mi_les_nusgs(miEngine::New().ctx, k_.size(), coeffs_.ck, nullptr, k_.data(), delta_().data(), nuSgs_.data()), "oneEqEddy::updateSubGridScaleFields");
    evaluateBoundary(nuSgs_, bnuSgs_, false);
}
void oneEqEddy::correct(const flowData& flow, scalar rDeltaT, const dictionary& kSolver, scalar kRelax)
{
    const label n = k_.size();
    scalargpuField G(n), sp(n), dk(n);
    const double* grad[9];
    gradArrays(flow.gradU, grad);
    miCheck(mi_les_k_terms(miEngine::New().ctx, n, coeffs_.ce, nullptr, nuSgs_.data(), grad, k_.data(), delta_().data(), nullptr, nu_, G.data(), sp.data(),
                           dk.data()), "oneEqEddy::correct");
    solveK(G, sp, dk, flow, rDeltaT, kRelax, kSolver);      // :106-119
    updateSubGridScaleFields();
}

dynOneEqEddy::dynOneEqEddy(const meshData& mesh, const flowData& flow, scalar nu, const scalargpuField& k, const scalargpuField& bk,
                           const dictionary& coeffDict, scalar kMin)
    : GenEddyVisc(mesh, nu, k, bk, coeffDict, kMin), simpleFilter_(*mesh.average, *mesh.weights), filter_(simpleFilter_)
{
    bound(k_, &bk_, *mesh_.average, *mesh_.weights, kMin_);   // dynOneEqEddy.C:134
    scalargpuField ck(k_.size()), ce(k_.size());
    coefficients(flow, false, ck, ce);                      // :136-137: KK is not clipped here
    updateSubGridScaleFields(ck);
}
void dynOneEqEddy::updateSubGridScaleFields(const scalargpuField& ck)
{
    miCheck(mi_les_nusgs(miEngine::New().ctx, k_.size(), 0.0, ck.data(), k_.data(), delta_().data(), nuSgs_.data()), "dynOneEqEddy::updateSubGridScaleFields");
    evaluateBoundary(nuSgs_, bnuSgs_, false);
}
void dynOneEqEddy::coefficients(const flowData& flow, bool clip, scalargpuField& ck, scalargpuField& ce) const
{
    const mi_ctx_t ctx = miEngine::New().ctx;
    const label n = k_.size(), nb = nb_;
    const char* who = "dynOneEqEddy::ck";
    // a field with its boundary: [0] the cells, [1] the patch-ordered boundary values
    auto fields = [&](int m) { return std::array<std::vector<scalargpuField>, 2>{std::vector<scalargpuField>((std::size_t)m, scalargpuField(n)),
                                                                                  std::vector<scalargpuField>((std::size_t)m, scalargpuField(nb))}; };
    // sqr(U) 0-5, magSqr(U) 6, D 7-12, magSqr(D) 13 (mi_les_dyn_moments), on the cells and on the boundary values
    auto mom = fields(14);
    for (int s = 0; s < 2; ++s) {
        const vectorgpuField& U = s ? *flow.bU : *flow.U;
        const double* u[3] = {U.component(0).data(), U.component(1).data(), U.component(2).data()};
        const double* grad[9];
        gradArrays(s ? flow.bGradU : flow.gradU, grad);
        double *sq[6], *D[6];
        dataOf(mom[s], 0, sq, 6); dataOf(mom[s], 7, D, 6);
        miCheck(mi_les_dyn_moments(ctx, s ? nb : n, u, grad, sq, mom[s][6].data(), D, mom[s][13].data()), who);
    }
    // filter_ : U 0-2, sqr(U) 3-8, magSqr(U) 9, D 10-15, magSqr(D) 16 -- each filtered field once, two launches
    auto f1 = fields(17);
    {
        std::vector<const scalargpuField*> in, bin;
        for (int s = 0; s < 2; ++s) {
            const vectorgpuField& U = s ? *flow.bU : *flow.U;
            std::vector<const scalargpuField*>& v = s ? bin : in;
            for (int d = 0; d < 3; ++d) v.push_back(&U.component((direction)d));
            for (const scalargpuField* x : cptrs(mom[s], 0, 6)) v.push_back(x);
        }
        filter_(in, bin, mptrs(f1[0], 0, 9));
        filter_(cptrs(mom[0], 6, 14), cptrs(mom[1], 6, 14), mptrs(f1[0], 9, 17));
    }
    for (int i = 0; i < 17; ++i) evaluateBoundary(f1[0][(std::size_t)i], f1[1][(std::size_t)i], false);
    // KK 0, LL 1-6, MM 7-12, ce_num 13, ce_den 14 (mi_les_dyn_level1); nuEff = nuSgs + nu, delta_b = SMALL
    auto lv = fields(15);
    scalargpuField nuEffC(n), nuEffB(nb), spC(n), spB(nb);
    miCheck(mi_ke_k_terms(ctx, n, k_.data(), k_.data(), nuSgs_.data(), nullptr, nu_, spC.data(), nuEffC.data()), who);
    miCheck(mi_ke_k_terms(ctx, nb, bk_.data(), bk_.data(), bnuSgs_.data(), nullptr, nu_, spB.data(), nuEffB.data()), who);
    for (int s = 0; s < 2; ++s) {
        const double *fU[3], *fS[6], *fD[6];
        dataOf(f1[s], 0, fU, 3); dataOf(f1[s], 3, fS, 6); dataOf(f1[s], 10, fD, 6);
        double *LL[6], *MM[6];
        dataOf(lv[s], 1, LL, 6); dataOf(lv[s], 7, MM, 6);
        miCheck(mi_les_dyn_level1(ctx, s ? nb : n, clip ? 1 : 0, (s ? delta_.boundaryField() : delta_()).data(), (s ? nuEffB : nuEffC).data(), fU, fS,
                                  f1[s][9].data(), fD, f1[s][16].data(), lv[s][0].data(), LL, MM, lv[s][13].data(), lv[s][14].data(), nullptr), who);
    }
    // simpleFilter_ : LL 0-5, MM 6-11, ce_num 12, ce_den 13
    auto f2 = fields(14);
    simpleFilter_(cptrs(lv[0], 1, 10), cptrs(lv[1], 1, 10), mptrs(f2[0], 0, 9));
    simpleFilter_(cptrs(lv[0], 10, 15), cptrs(lv[1], 10, 15), mptrs(f2[0], 9, 14));
    for (int i = 0; i < 12; ++i) evaluateBoundary(f2[0][(std::size_t)i], f2[1][(std::size_t)i], false);
    auto lm = fields(2);
    for (int s = 0; s < 2; ++s) {
        const double *fLL[6], *fMM[6];
        dataOf(f2[s], 0, fLL, 6); dataOf(f2[s], 6, fMM, 6);
        miCheck(mi_les_dyn_level2(ctx, s ? nb : n, fLL, fMM, lm[s][0].data(), lm[s][1].data()), who);
    }
    auto f3 = fields(2);
    simpleFilter_(cptrs(lm[0], 0, 2), cptrs(lm[1], 0, 2), mptrs(f3[0], 0, 2));
    miCheck(mi_les_dyn_coeffs(ctx, n, f3[0][0].data(), f3[0][1].data(), f2[0][12].data(), f2[0][13].data(), ck.data(), ce.data()), who);
}
void dynOneEqEddy::correct(const flowData& flow, scalar rDeltaT, const dictionary& kSolver, scalar kRelax)
{
    const label n = k_.size();
    scalargpuField ck(n), ce(n), P(n), sp(n), dk(n);
    coefficients(flow, true, ck, ce);                       // :151-152 and the ck / ce of :163, :171
    const double* grad[9];
    gradArrays(flow.gradU, grad);
    miCheck(mi_les_k_terms(miEngine::New().ctx, n, 0.0, ce.data(), nuSgs_.data(), grad, k_.data(), delta_().data(), nullptr, nu_, P.data(), sp.data(), dk.data()),
            "dynOneEqEddy::correct");
    solveK(P, sp, dk, flow, rDeltaT, kRelax, kSolver);      // :154-169
    updateSubGridScaleFields(ck);
}
}
}
void interfaceProperties::sigmaK(scalargpuField& out) const { fieldAxpby(out, sigma_, K_, 0.0, K_); }
void interfaceProperties::surfaceTensionForce(scalargpuField& out, const scalargpuField& alpha1, const scalargpuField* snGradCorr) const
{
    miCheck(mi_surface_tension_force(mesh_.addr->handle(), sigma_, mesh_.weights->data(), mesh_.deltaCoeffs->data(), K_.data(), alpha1.data(),
                                     snGradCorr ? snGradCorr->data() : nullptr, out.data()), "interfaceProperties::surfaceTensionForce");
}
void interfaceProperties::patchSurfaceTensionForce(scalargpuField& out, label patchi, const scalargpuField& pDeltaCoeffs, const scalargpuField& nbrK,
                                                   const scalargpuField& alpha1, const scalargpuField& nbrAlpha1, const scalargpuField* pSnGradCorr) const
{
    const patchData& p = patches_[(size_t)patchi];
    if (!p.weights) FatalErrorIn("interfaceProperties::surfaceTensionForce", "the patch is not coupled: the product of two boundary fields is the caller's");
    miCheck(mi_patch_surface_tension_force(p.cells->handle(), sigma_, p.weights->data(), pDeltaCoeffs.data(), K_.data(), nbrK.data(), alpha1.data(),
                                           nbrAlpha1.data(), pSnGradCorr ? pSnGradCorr->data() : nullptr, out.data()),
            "interfaceProperties::surfaceTensionForce (coupled patch)");
}
void interfaceProperties::nearInterface(scalargpuField& out, const scalargpuField& alpha1) const
{
    miCheck(mi_near_interface(miEngine::New().ctx, alpha1.size(), alpha1.data(), out.data()), "interfaceProperties::nearInterface");
}
void interfaceProperties::calculateK(const vectorgpuField& gradAlpha, const std::vector<const vectorgpuField*>& bGradAlpha,
                                     const std::vector<scalargpuField*>& gradientOut)
{
    if (bGradAlpha.size() != patches_.size()) FatalErrorIn("interfaceProperties::calculateK", "one boundary gradient per patch");
    const auto sf = cmptData(*mesh_.Sf);
    const auto g = cmptData(gradAlpha);
    miCheck(mi_interface_nhatf(mesh_.addr->handle(), deltaN_, mesh_.weights->data(), sf, g, nHatf_.data(), nullptr), "interfaceProperties::calculateK");
    label off = 0;
    for (size_t i = 0; i < patches_.size(); ++i) {
        const patchData& p = patches_[i];
        mi_patch_nhatf x{};
        const auto ps = cmptData(*p.Sf);
        const auto bg = cmptData(*bGradAlpha[i]);
        for (int d = 0; d < 3; ++d) {
            x.patch_sf_dev[d] = ps[d];
            x.grad_dev[d] = p.weights ? g[d] : bg[d];
            x.nbr_grad_dev[d] = p.weights ? bg[d] : nullptr;
        }
        x.patch_weights_dev = p.weights ? p.weights->data() : nullptr;
        if (p.thetaDeg) {                             // correctContactAngle (:69-114)
            x.theta_deg_dev = p.thetaDeg->data();
            x.patch_magsf_dev = p.magSf ? p.magSf->data() : nullptr;
            if (i < gradientOut.size() && gradientOut[i]) x.gradient_out_dev = gradientOut[i]->data();
        }
        x.nhatf_out_dev = nHatfb_.data() + off;
        miCheck(mi_patch_interface_nhatf(p.cells->handle(), deltaN_, &x), "interfaceProperties::calculateK (patch)");
        off += p.cells->size();
    }
    miCheck(mi_interface_curvature(h_, nHatf_.data(), nHatfb_.data(), mesh_.V->data(), K_.data()), "interfaceProperties::calculateK (K)");
}
void interfaceProperties::correct(const vectorgpuField& gradAlpha, const std::vector<const vectorgpuField*>& bGradAlpha,
                                  const std::vector<scalargpuField*>& gradientOut)
{
    calculateK(gradAlpha, bGradAlpha, gradientOut);
}

// ---- Pstream: the parallel run as this path sees it -------------------------------------------------------------
namespace {
struct PstreamState { bool par = false; int rank = 0, n = 1; mi_comm_t red = nullptr, halo = nullptr; };
PstreamState& pstream() { static PstreamState s; return s; }
}
bool Pstream::parRun() { return pstream().par; }
int Pstream::myProcNo() { return pstream().rank; }
int Pstream::nProcs() { return pstream().n; }
mi_comm_t Pstream::reduceComm() { return pstream().red; }
mi_comm_t Pstream::haloComm() { return pstream().halo; }
void Pstream::init(int myProcNo, int nProcs, const std::string& idFile)
{
    PstreamState& P = pstream();
    if (P.par) FatalErrorIn("Pstream::init", "already initialised");
    if (nProcs < 1 || myProcNo < 0 || myProcNo >= nProcs) FatalErrorIn("Pstream::init", "bad rank / size");
    unsigned char ids[256];
    if (myProcNo == 0) {
        miCheck(mi_comm_unique_id(ids, 128), "Pstream::init");
        miCheck(mi_comm_unique_id(ids + 128, 128), "Pstream::init");
        if (nProcs > 1) { // publish atomically: write beside, then rename
            const std::string tmp = idFile + ".tmp";
            FILE* f = fopen(tmp.c_str(), "wb");
            if (!f || fwrite(ids, 1, 256, f) != 256) FatalErrorIn("Pstream::init", "cannot write " + tmp);
            fclose(f);
            if (rename(tmp.c_str(), idFile.c_str()) != 0) FatalErrorIn("Pstream::init", "cannot publish " + idFile);
        }
    } else {
        bool got = false;
        for (int attempt = 0; attempt < 6000 && !got; ++attempt) { // up to ~10 min
            FILE* f = fopen(idFile.c_str(), "rb");
            if (f) { got = fread(ids, 1, 256, f) == 256; fclose(f); }
            if (!got) { struct timespec ts = {0, 100 * 1000 * 1000}; nanosleep(&ts, nullptr); }
        }
        if (!got) FatalErrorIn("Pstream::init", "rank 0 never published the communicator ids in " + idFile);
    }
    mi_ctx_t ctx = miEngine::New().ctx;
    miCheck(mi_comm_create(ctx, nProcs, myProcNo, ids, &P.red), "Pstream::init");
    miCheck(mi_comm_create(ctx, nProcs, myProcNo, ids + 128, &P.halo), "Pstream::init");
    P.par = true; P.rank = myProcNo; P.n = nProcs;
}
void Pstream::exit()
{
    PstreamState& P = pstream();
    if (P.halo) mi_comm_destroy(P.halo);
    if (P.red) mi_comm_destroy(P.red);
    P = PstreamState();
}
scalar Pstream::returnReduceSum(scalar v)
{
    if (!parRun()) return v;
    scalargpuField t(1);
    t = scalarField(1, v);
    miCheck(mi_comm_allreduce_sum(reduceComm(), t.data(), 1), "returnReduce");
    return t.asHost()[0];
}
label Pstream::returnReduceSum(label v)
{
    if (!parRun()) return v;
    scalargpuField t(1);
    t = scalarField(1, (scalar)v);
    miCheck(mi_comm_allreduce_sum(reduceComm(), t.data(), 1), "returnReduce");
    return (label)(t.asHost()[0] + 0.5);
}

// ---- the limited gradient schemes -------------------------------------------------------------------------------------------------
fv::limitedGradScheme fv::limitedGradScheme::New(const std::string& scheme)
{
    mi_grad_limiter l{};
    miCheck(mi_grad_limiter_parse(scheme.c_str(), &l), "gradScheme::New");
    return limitedGradScheme(l);
}
// ---- the snGrad schemes ---------------------------------------------------------------------------------------------------------------
fv::snGradScheme fv::snGradScheme::New(const std::string& scheme)
{
    mi_sngrad_scheme s{};
    miCheck(mi_sngrad_parse(scheme.c_str(), &s), "snGradScheme::New");
    return snGradScheme(s);
}
fv::snGradScheme fv::snGradScheme::laplacian(const std::string& where, const std::string& term, const std::vector<std::string>& scheme,
                                             const std::function<std::vector<std::string>()>& snGradEntry)
{
    const std::string forms = "laplacianSchemes " + term + ": Gauss linear corrected | uncorrected | orthogonal | limited [corrected] <k>";
    if (scheme.size() < 3 || scheme[0] != "Gauss" || scheme[1] != "linear") FatalErrorIn(where, forms);
    std::string tail;
    for (std::size_t i = 2; i < scheme.size(); ++i) tail += (i > 2 ? " " : "") + scheme[i];
    mi_sngrad_scheme s{};
    if (mi_sngrad_parse(tail.c_str(), &s) != 0) FatalErrorIn(where, forms + " (" + mi_last_error() + ")");
    if (s.kind == MI_SNGRAD_LIMITED) {
        const std::vector<std::string> words = snGradEntry();
        std::string entry;
        for (std::size_t i = 0; i < words.size(); ++i) entry += (i ? " " : "") + words[i];
        mi_sngrad_scheme e{};
        if (mi_sngrad_parse(entry.c_str(), &e) != 0 || e.kind != s.kind || e.limit_coeff != s.limit_coeff)
            FatalErrorIn(where, forms + " ('" + tail + "' needs the same snGradSchemes entry; that one says '" + entry + "')");
    }
    return snGradScheme(s);
}
void fvc::snGradLimitedCorrectionFlux(scalargpuField& flux, const lduAddressing& a, const fv::snGradScheme& s, const vectorgpuField& corrVecs,
                                      const scalargpuField& weights, const scalargpuField& deltaCoeffs, const scalargpuField& vf, const vectorgpuField& gradVf,
                                      const scalargpuField& gammaMagSf, scalargpuField* limiter)
{
    if (!s.limited()) FatalErrorIn("fvc::snGradLimitedCorrectionFlux", "the scheme is not `limited`");
    const double* v[1] = {vf.data()};
    const auto g = cmptData(gradVf);
    double* out[1] = {flux.data()};
    miCheck(mi_sngrad_limited_correction_flux(a.handle(), 1, s.limitCoeff(), corrVecs.component(0).data(), corrVecs.component(1).data(),
                                              corrVecs.component(2).data(), weights.data(), deltaCoeffs.data(), v, g, gammaMagSf.data(), out,
                                              limiter ? limiter->data() : nullptr), "limitedSnGrad::correction");
}
void fvc::snGradLimitedCorrectionFlux(vectorgpuField& flux, const lduAddressing& a, const fv::snGradScheme& s, const vectorgpuField& corrVecs,
                                      const scalargpuField& weights, const scalargpuField& deltaCoeffs, const vectorgpuField& vf,
                                      const vectorgpuField* const gradVf[3], const scalargpuField& gammaMagSf, scalargpuField* limiter)
{
    if (!s.limited()) FatalErrorIn("fvc::snGradLimitedCorrectionFlux", "the scheme is not `limited`");
    const double *v[3], *g[9];
    double* out[3];
    for (int j = 0; j < 3; ++j) {
        v[j] = vf.component(j).data(); out[j] = flux.component(j).data();
        for (int d = 0; d < 3; ++d) g[3 * j + d] = gradVf[j]->component(d).data();
    }
    miCheck(mi_sngrad_limited_correction_flux(a.handle(), 3, s.limitCoeff(), corrVecs.component(0).data(), corrVecs.component(1).data(),
                                              corrVecs.component(2).data(), weights.data(), deltaCoeffs.data(), v, g, gammaMagSf.data(), out,
                                              limiter ? limiter->data() : nullptr), "limitedSnGrad::correction");
}
// ---- divDevReff's explicit term -------------------------------------------------------------------------------------------------------
void fvc::gaussGradBoundary(vectorgpuField& gb, const fvPatchCells& p, const vectorgpuField& pSf, const scalargpuField& pMagSf, const scalargpuField& pSnGrad,
                            const vectorgpuField& gradVf)
{
    const double* sn[1] = {pSnGrad.data()};
    const auto g = cmptData(gradVf);
    const auto out = cmptData(gb);
    miCheck(mi_patch_gauss_grad_correct(p.handle(), 1, pSf.component(0).data(), pSf.component(1).data(), pSf.component(2).data(), pMagSf.data(), sn, g, out),
            "gaussGrad::correctBoundaryConditions");
}
void fvc::gaussGradBoundary(vectorgpuField* const gb[3], const fvPatchCells& p, const vectorgpuField& pSf, const scalargpuField& pMagSf,
                            const vectorgpuField& pSnGrad, const vectorgpuField* const gradVf[3])
{
    const double *sn[3], *g[9];
    double* out[9];
    for (int j = 0; j < 3; ++j) {
        sn[j] = pSnGrad.component(j).data();
        for (int k = 0; k < 3; ++k) { g[3 * j + k] = gradVf[j]->component(k).data(); out[3 * j + k] = gb[j]->component(k).data(); }
    }
    miCheck(mi_patch_gauss_grad_correct(p.handle(), 3, pSf.component(0).data(), pSf.component(1).data(), pSf.component(2).data(), pMagSf.data(), sn, g, out),
            "gaussGrad::correctBoundaryConditions");
}
void fvc::divDevTGrad(vectorgpuField& div, const lduAddressing& a, devKind kind, const scalargpuField& weights, const vectorgpuField& Sf,
                      const scalargpuField& visc, const vectorgpuField* const gradU[3], const std::vector<devTGradPatch>& patches, const scalargpuField& V,
                      vectorgpuField* faceFlux)
{
    auto nine = [](const vectorgpuField* const g[3], const double* out[9]) {
        for (int j = 0; j < 3; ++j) for (int k = 0; k < 3; ++k) out[3 * j + k] = g[j]->component(k).data();
    };
    const double* g[9];
    nine(gradU, g);
    vectorgpuField own(faceFlux ? 0 : weights.size());
    vectorgpuField& ff = faceFlux ? *faceFlux : own;
    const auto face = cmptData(ff);
    const auto sum = cmptData(div);
    miCheck(mi_fvc_div_dev_tgrad(a.handle(), kind, weights.data(), Sf.component(0).data(), Sf.component(1).data(), Sf.component(2).data(), visc.data(), g,
                                 nullptr, face, sum), "fvc::div(visc*dev(T(grad(U))))");
    for (const devTGradPatch& p : patches) {                    // the boundary faces, in patch order (fvcSurfaceIntegrate.C:58-72)
        const label np = p.cells->size();
        if (np == 0) continue;
        vectorgpuField pf(np);
        const auto out = cmptData(pf);
        const double *pg[9], *ng[9];
        if (p.weights) { nine(p.nbrGrad, ng); for (int i = 0; i < 9; ++i) pg[i] = g[i]; }
        else nine(p.grad, pg);
        miCheck(mi_patch_dev_tgrad_flux(p.cells->handle(), kind, p.Sf->component(0).data(), p.Sf->component(1).data(), p.Sf->component(2).data(),
                                        p.weights ? p.weights->data() : nullptr, p.weights ? visc.data() : p.visc->data(), pg,
                                        p.weights ? p.nbrVisc->data() : nullptr, p.weights ? ng : nullptr, out), "fvc::div(visc*dev(T(grad(U)))) (patch)");
        for (direction d = 0; d < 3; ++d) p.cells->add(pf.component(d), div.component(d));
    }
    for (direction d = 0; d < 3; ++d) fieldDivide(div.component(d), div.component(d), V);
}
void fvVectorMatrix::subtractField(const vectorgpuField& vf, const scalargpuField& V)
{
    mi_ctx_t ctx = miEngine::New().ctx;
    scalargpuField neg(V.size());
    for (direction d = 0; d < 3; ++d) {
        miCheck(mi_vec_axpby(ctx, V.size(), -1.0, vf.component(d).data(), 0.0, vf.component(d).data(), neg.data()), "fvMatrix - field: -field");
        miCheck(mi_fvm_su(ctx, V.size(), V.data(), neg.data(), source_.component(d).data()), "fvMatrix - field: source += V*field");
    }
}
gradBoundary::gradBoundary(const lduAddressing& a, const std::vector<labelList>& faceCells, const std::vector<patchKind>& kinds) : h_(nullptr)
{
    if (faceCells.size() != kinds.size()) FatalErrorIn("gradBoundary", "one kind per patch");
    std::vector<int32_t> sizes, kd;
    std::vector<const int32_t*> ptrs;
    for (size_t p = 0; p < faceCells.size(); ++p) {
        sizes.push_back((int32_t)faceCells[p].size()); ptrs.push_back(faceCells[p].data()); kd.push_back((int32_t)kinds[p]);
    }
    miCheck(mi_grad_boundary_create(a.handle(), (int32_t)sizes.size(), sizes.data(), ptrs.data(), kd.data(), &h_), "gradBoundary");
}
gradBoundary::~gradBoundary() { if (h_) mi_grad_boundary_destroy(h_); }
void fvc::limitedGrad(vectorgpuField& g, const lduAddressing& a, const fv::limitedGradScheme& s, const gradBoundary* b, const scalargpuField& vf,
                      const vectorgpuField& C, const vectorgpuField& Cf, const scalargpuField* bValue, const vectorgpuField* bCf, scalargpuField* limiter)
{
    const double* v[1] = {vf.data()};
    const auto c = cmptData(C);
    const auto cf = cmptData(Cf);
    const double* bv[1] = {bValue ? bValue->data() : nullptr};
    const double* bcf[3] = {nullptr, nullptr, nullptr};
    if (bCf) for (int d = 0; d < 3; ++d) bcf[d] = bCf->component(d).data();
    const auto gr = cmptData(g);
    double* lim[1] = {limiter ? limiter->data() : nullptr};
    miCheck(mi_limited_grad(a.handle(), &s.data(), b ? b->handle() : nullptr, 1, v, c, cf, bValue ? bv : nullptr, bCf ? bcf : nullptr, gr,
                            limiter ? lim : nullptr), "fvc::grad (limited)");
}
void fvc::limitedGrad(vectorgpuField* const g[3], const lduAddressing& a, const fv::limitedGradScheme& s, const gradBoundary* b, const vectorgpuField& vf,
                      const vectorgpuField& C, const vectorgpuField& Cf, const vectorgpuField* bValue, const vectorgpuField* bCf, vectorgpuField* limiter)
{
    const double *v[3], *c[3], *cf[3], *bv[3] = {nullptr, nullptr, nullptr}, *bcf[3] = {nullptr, nullptr, nullptr};
    double *gr[9], *lim[3] = {nullptr, nullptr, nullptr};
    for (int d = 0; d < 3; ++d) {
        v[d] = vf.component(d).data(); c[d] = C.component(d).data(); cf[d] = Cf.component(d).data();
        if (bValue) bv[d] = bValue->component(d).data();
        if (bCf) bcf[d] = bCf->component(d).data();
        if (limiter) lim[d] = limiter->component(d).data();
        for (int k = 0; k < 3; ++k) gr[3 * d + k] = g[d]->component(k).data();
    }
    miCheck(mi_limited_grad(a.handle(), &s.data(), b ? b->handle() : nullptr, 3, v, c, cf, bValue ? bv : nullptr, bCf ? bcf : nullptr, gr,
                            limiter ? lim : nullptr), "fvc::grad (limited)");
}

// ---- the leastSquares gradient scheme ----------------------------------------------------------------------------------------------
fv::gradScheme fv::gradScheme::New(const std::string& entry)
{
    mi_grad_scheme s{};
    miCheck(mi_grad_scheme_parse(entry.c_str(), &s), "gradScheme::New");
    return gradScheme(s);
}
fv::limitedGradScheme fv::gradScheme::limiter() const
{
    if (!s_.limited) FatalErrorIn("gradScheme::limiter", "the gradient scheme is not a limited one");
    return limitedGradScheme(s_.limiter);
}
leastSquaresVectors::leastSquaresVectors(const lduAddressing& a, const gradBoundary* b, const vectorgpuField& C, const scalargpuField& weights,
                                         const scalargpuField& magSf, const scalargpuField* bWeights, const scalargpuField* bMagSf,
                                         const vectorgpuField* bDelta)
    : h_(nullptr), nFaces_(weights.size()), nBFaces_(bMagSf ? bMagSf->size() : 0)
{
    const auto c = cmptData(C);
    const double* bd[3] = {nullptr, nullptr, nullptr};
    if (bDelta) for (int d = 0; d < 3; ++d) bd[d] = bDelta->component(d).data();
    miCheck(mi_ls_vectors_create(a.handle(), b ? b->handle() : nullptr, c, weights.data(), magSf.data(), bWeights ? bWeights->data() : nullptr,
                                 bMagSf ? bMagSf->data() : nullptr, bDelta ? bd : nullptr, &h_), "leastSquaresVectors::New");
}
leastSquaresVectors::~leastSquaresVectors() { if (h_) mi_ls_vectors_destroy(h_); }
void leastSquaresVectors::fields(vectorgpuField& pVectors, vectorgpuField& nVectors, vectorgpuField* bPVectors) const
{
    if (pVectors.size() != nFaces_ || nVectors.size() != nFaces_ || (bPVectors && bPVectors->size() != nBFaces_))
        FatalErrorIn("leastSquaresVectors::fields", "the fields have another size than the mesh's faces");
    const auto p = cmptData(pVectors);
    const auto n = cmptData(nVectors);
    double* bp[3] = {nullptr, nullptr, nullptr};
    if (bPVectors) for (int d = 0; d < 3; ++d) bp[d] = bPVectors->component(d).data();
    miCheck(mi_ls_vectors_fields(h_, p, n, bPVectors ? bp : nullptr), "leastSquaresVectors::fields");
}
void fvc::leastSquaresGrad(vectorgpuField& g, const leastSquaresVectors& lsv, const scalargpuField& vf, const scalargpuField* bValue)
{
    const double* v[1] = {vf.data()};
    const double* bv[1] = {bValue ? bValue->data() : nullptr};
    const auto gr = cmptData(g);
    miCheck(mi_ls_grad(lsv.handle(), 1, v, bValue ? bv : nullptr, gr), "fvc::grad (leastSquares)");
}
void fvc::leastSquaresGrad(vectorgpuField* const g[3], const leastSquaresVectors& lsv, const vectorgpuField& vf, const vectorgpuField* bValue)
{
    const double *v[3], *bv[3] = {nullptr, nullptr, nullptr};
    double* gr[9];
    for (int d = 0; d < 3; ++d) {
        v[d] = vf.component(d).data();
        if (bValue) bv[d] = bValue->component(d).data();
        for (int k = 0; k < 3; ++k) gr[3 * d + k] = g[d]->component(k).data();
    }
    miCheck(mi_ls_grad(lsv.handle(), 3, v, bValue ? bv : nullptr, gr), "fvc::grad (leastSquares)");
}

// ---- fvc::surfaceSum and fvc::reconstruct ------------------------------------------------------------------------------------------------
reconstructData::reconstructData(const lduAddressing& a, const gradBoundary* b, const vectorgpuField& Sf, const scalargpuField& magSf,
                                 const vectorgpuField* bSf, const scalargpuField* bMagSf)
    : h_(nullptr), nCells_(a.size())
{
    const auto s = cmptData(Sf);
    const double* bs[3] = {nullptr, nullptr, nullptr};
    if (bSf) for (int d = 0; d < 3; ++d) bs[d] = bSf->component(d).data();
    miCheck(mi_reconstruct_create(a.handle(), b ? b->handle() : nullptr, s, magSf.data(), bSf ? bs : nullptr, bMagSf ? bMagSf->data() : nullptr, &h_),
            "reconstructData::New");
}
reconstructData::~reconstructData() { if (h_) mi_reconstruct_destroy(h_); }
void reconstructData::fields(scalargpuField* const inv[9], int removed[3]) const
{
    double* out[9];
    for (int i = 0; i < 9; ++i) {
        if (!inv[i] || inv[i]->size() != nCells_) FatalErrorIn("reconstructData::fields", "the fields have another size than the mesh's cells");
        out[i] = inv[i]->data();
    }
    int32_t rm[3] = {0, 0, 0};
    miCheck(mi_reconstruct_fields(h_, out, rm), "reconstructData::fields");
    if (removed) for (int d = 0; d < 3; ++d) removed[d] = rm[d];
}
void fvc::surfaceSum(scalargpuField& out, const lduAddressing& a, const scalargpuField& ssf, bool mag)
{
    miCheck(mi_surface_sum(a.handle(), mag ? MI_SURFACE_SUM_MAG : MI_SURFACE_SUM, ssf.data(), out.data()), "fvc::surfaceSum");
}
void fvc::surfaceSumPatch(scalargpuField& out, const fvPatchCells& p, const scalargpuField& pssf, bool mag)
{
    if (p.size()) miCheck(mi_patch_add(p.handle(), pssf.data(), out.data(), mag ? 2 : 0), "fvc::surfaceSum (patch)");
}
void fvc::reconstruct(vectorgpuField& out, const reconstructData& rc, const scalargpuField& ssf, const scalargpuField* bssf)
{
    vectorgpuField* const o[1] = {&out};
    const scalargpuField* const s[1] = {&ssf};
    const scalargpuField* const b[1] = {bssf};
    reconstruct(o, rc, 1, s, bssf ? b : nullptr);
}
void fvc::reconstruct(vectorgpuField* const out[], const reconstructData& rc, label n, const scalargpuField* const ssf[], const scalargpuField* const bssf[])
{
    if (n < 1 || n > 4) FatalErrorIn("fvc::reconstruct", "1 to 4 fluxes in one call");
    const double *s[4], *b[4];
    double* o[12];
    for (label r = 0; r < n; ++r) {
        s[r] = ssf[r]->data();
        b[r] = bssf ? bssf[r]->data() : nullptr;
        for (int k = 0; k < 3; ++k) o[3 * r + k] = out[r]->component(k).data();
    }
    miCheck(mi_fvc_reconstruct(rc.handle(), (int32_t)n, s, bssf ? b : nullptr, o), "fvc::reconstruct");
}

// ---- explicit MULES ---------------------------------------------------------------------------------------------------------------------
mulesData::mulesData(const lduAddressing& a, const gradBoundary* b, const std::vector<bool>& wedge)
    : h_(nullptr), nFaces_((label)a.lowerAddrHost().size()), nBFaces_(0)
{
    std::vector<int32_t> w(wedge.begin(), wedge.end());
    miCheck(mi_mules_create(a.handle(), b ? b->handle() : nullptr, w.empty() ? nullptr : w.data(), &h_), "mulesData::New");
}
mulesData::~mulesData() { if (h_) mi_mules_destroy(h_); }
scalargpuField& mulesData::work(int i) const
{
    if (!work_[i]) work_[i].reset(new scalargpuField(i % 2 == 0 ? nFaces_ : nBFaces_));
    return *work_[i];
}
namespace {
mi_mules_fields mulesFields(const MULES::rDeltaTType& rDeltaT, const MULES::rhoType& rho, const MULES::volField& psi, const scalargpuField* Sp,
                            const scalargpuField* Su, const scalargpuField& V, scalar psiMax, scalar psiMin)
{
    mi_mules_fields f{};
    f.r_delta_t = rDeltaT.value; f.r_delta_t_dev = rDeltaT.field ? rDeltaT.field->data() : nullptr;
    f.rho_dev = rho.field ? rho.field->data() : nullptr; f.rho_old_dev = rho.oldTime ? rho.oldTime->data() : nullptr;
    f.sp_dev = Sp ? Sp->data() : nullptr; f.su_dev = Su ? Su->data() : nullptr;
    f.vol_dev = V.data(); f.psi_dev = psi.field ? psi.field->data() : nullptr; f.psi_old_dev = psi.oldTime ? psi.oldTime->data() : nullptr;
    f.b_psi_dev = psi.boundary ? psi.boundary->data() : nullptr;
    f.psi_max = psiMax; f.psi_min = psiMin;
    return f;
}
double* dataOf(scalargpuField* f) { return f ? f->data() : nullptr; }
}
void MULES::limiter(const mulesData& m, surfaceField allLambda, const rDeltaTType& rDeltaT, const rhoType& rho, const volField& psi,
                    const surfaceField& phiBD, const surfaceField& phiCorr, const scalargpuField* Sp, const scalargpuField* Su, const scalargpuField& V,
                    scalar psiMax, scalar psiMin, label nLimiterIter)
{
    const mi_mules_fields f = mulesFields(rDeltaT, rho, psi, Sp, Su, V, psiMax, psiMin);
    mi_mules_flux x{};
    x.phi_bd_dev = dataOf(phiBD.field); x.b_phi_bd_dev = dataOf(phiBD.boundary);
    x.phi_corr_dev = dataOf(phiCorr.field); x.b_phi_corr_dev = dataOf(phiCorr.boundary);
    x.lambda_dev = dataOf(allLambda.field); x.b_lambda_dev = dataOf(allLambda.boundary);
    miCheck(mi_mules_limiter(m.handle(), (int32_t)nLimiterIter, &f, &x), "MULES::limiter");
}
void MULES::limit(const mulesData& m, const rDeltaTType& rDeltaT, const rhoType& rho, const volField& psi, const surfaceField& phi, surfaceField phiPsi,
                  const scalargpuField* Sp, const scalargpuField* Su, const scalargpuField& V, scalar psiMax, scalar psiMin, label nLimiterIter,
                  bool returnCorr)
{
    const mi_mules_fields f = mulesFields(rDeltaT, rho, psi, Sp, Su, V, psiMax, psiMin);
    const bool hasB = phiPsi.boundary != nullptr;
    mi_mules_flux x{};
    x.phi_dev = dataOf(phi.field); x.b_phi_dev = dataOf(phi.boundary);
    x.phi_psi_dev = dataOf(phiPsi.field); x.b_phi_psi_dev = dataOf(phiPsi.boundary);
    x.phi_bd_dev = m.work(0).data(); x.phi_corr_dev = m.work(2).data(); x.lambda_dev = m.work(4).data();
    if (hasB) {
        const label nb = phiPsi.boundary->size();
        for (int i = 1; i < 6; i += 2) if (m.work(i).size() != nb) m.work(i) = scalargpuField(nb);
        x.b_phi_bd_dev = m.work(1).data(); x.b_phi_corr_dev = m.work(3).data(); x.b_lambda_dev = m.work(5).data();
    }
    x.out_dev = dataOf(phiPsi.field); x.b_out_dev = dataOf(phiPsi.boundary);    // the reference overwrites phiPsi
    miCheck(mi_mules_limit(m.handle(), (int32_t)nLimiterIter, returnCorr ? 1 : 0, &f, &x), "MULES::limit");
}
void MULES::explicitSolve(const mulesData& m, const rDeltaTType& rDeltaT, const rhoType& rho, const volField& psi, const surfaceField& phiPsi,
                          const scalargpuField* Sp, const scalargpuField* Su, const scalargpuField& V)
{
    const mi_mules_fields f = mulesFields(rDeltaT, rho, psi, Sp, Su, V, 0, 0);
    miCheck(mi_mules_explicit_solve(m.handle(), &f, dataOf(phiPsi.field), dataOf(phiPsi.boundary), dataOf(psi.field)), "MULES::explicitSolve");
}
void MULES::explicitSolve(const mulesData& m, const rDeltaTType& rDeltaT, const rhoType& rho, const volField& psi, const surfaceField& phi,
                          surfaceField phiPsi, const scalargpuField* Sp, const scalargpuField* Su, const scalargpuField& V, scalar psiMax, scalar psiMin)
{
    limit(m, rDeltaT, rho, psi, phi, phiPsi, Sp, Su, V, psiMax, psiMin, 3, false);
    explicitSolve(m, rDeltaT, rho, psi, phiPsi, Sp, Su, V);
}
// ---- semi-implicit MULES ----
void MULES::limiterCorr(const mulesData& m, surfaceField allLambda, const rDeltaTType& rDeltaT, const rhoType& rho, const volField& psi,
                        const surfaceField& phi, const surfaceField& phiCorr, const scalargpuField* Sp, const scalargpuField* Su, const scalargpuField& V,
                        scalar psiMax, scalar psiMin, label nLimiterIter, scalar extremaCoeff)
{
    const mi_mules_fields f = mulesFields(rDeltaT, rho, psi, Sp, Su, V, psiMax, psiMin);
    mi_mules_flux x{};
    x.b_phi_dev = dataOf(phi.boundary);
    x.phi_corr_dev = dataOf(phiCorr.field); x.b_phi_corr_dev = dataOf(phiCorr.boundary);
    x.lambda_dev = dataOf(allLambda.field); x.b_lambda_dev = dataOf(allLambda.boundary);
    miCheck(mi_mules_limiter_corr(m.handle(), (int32_t)nLimiterIter, extremaCoeff, &f, &x), "MULES::limiterCorr");
}
void MULES::limitCorr(const mulesData& m, const rDeltaTType& rDeltaT, const rhoType& rho, const volField& psi, const surfaceField& phi, surfaceField phiCorr,
                      const scalargpuField* Sp, const scalargpuField* Su, const scalargpuField& V, scalar psiMax, scalar psiMin, label nLimiterIter,
                      scalar extremaCoeff)
{
    const mi_mules_fields f = mulesFields(rDeltaT, rho, psi, Sp, Su, V, psiMax, psiMin);
    mi_mules_flux x{};
    x.b_phi_dev = dataOf(phi.boundary);
    x.phi_corr_dev = dataOf(phiCorr.field); x.b_phi_corr_dev = dataOf(phiCorr.boundary);
    x.lambda_dev = m.work(4).data();
    if (phiCorr.boundary) {
        const label nb = phiCorr.boundary->size();
        if (m.work(5).size() != nb) m.work(5) = scalargpuField(nb);
        x.b_lambda_dev = m.work(5).data();
    }
    miCheck(mi_mules_limit_corr(m.handle(), (int32_t)nLimiterIter, extremaCoeff, &f, &x), "MULES::limitCorr");
}
void MULES::correct(const mulesData& m, const rDeltaTType& rDeltaT, const rhoType& rho, const volField& psi, const surfaceField&, const surfaceField& phiCorr,
                    const scalargpuField* Sp, const scalargpuField* Su, const scalargpuField& V)
{
    const mi_mules_fields f = mulesFields(rDeltaT, rho, psi, Sp, Su, V, 0, 0);
    miCheck(mi_mules_correct(m.handle(), &f, dataOf(phiCorr.field), dataOf(phiCorr.boundary), dataOf(psi.field)), "MULES::correct");
}
void MULES::correct(const mulesData& m, const rhoType& rho, const volField& psi, const surfaceField& phi, surfaceField phiCorr, const scalargpuField* Sp,
                    const scalargpuField* Su, const scalargpuField& V, scalar psiMax, scalar psiMin, const rDeltaTType& rDeltaT, label nLimiterIter,
                    scalar extremaCoeff)
{
    limitCorr(m, rDeltaT, rho, psi, phi, phiCorr, Sp, Su, V, psiMax, psiMin, nLimiterIter, extremaCoeff);
    correct(m, rDeltaT, rho, psi, phi, phiCorr, Sp, Su, V);
}

// ---- steadyState, localEuler, CoEuler and the bounded convection scheme ----
namespace {
mi_ddt_local_scheme parseLocal(const std::string& scheme, int kind, const char* name)
{
    mi_ddt_local_scheme s{};
    miCheck(mi_ddt_local_parse(scheme.c_str(), &s), "ddtSchemes");
    if (s.kind != kind) FatalErrorIn("ddtSchemes", "'" + scheme + "' is not " + name);
    return s;
}
}
fv::steadyStateDdtScheme fv::steadyStateDdtScheme::New(const std::string& scheme)
{
    parseLocal(scheme, MI_DDT_STEADY_STATE, "steadyState");
    return steadyStateDdtScheme();
}
fv::localEulerDdtScheme fv::localEulerDdtScheme::New(const std::string& scheme)
{
    return localEulerDdtScheme(parseLocal(scheme, MI_DDT_LOCAL_EULER, "localEuler").name);
}
void fv::localEulerDdtScheme::bind(const word& name, const scalargpuField& rDeltaT)
{
    if (name != rDeltaTName_) FatalErrorIn("localEulerDdtScheme", "the scheme reads the field '" + rDeltaTName_ + "', not '" + name + "'");
    field_ = &rDeltaT;
}
const scalargpuField& fv::localEulerDdtScheme::localRDeltaT() const
{
    if (!field_) FatalErrorIn("localEulerDdtScheme", "no field '" + rDeltaTName_ + "' (bind it first)");
    return *field_;
}
const scalargpuField* fv::localEulerDdtScheme::rDeltaT(label nCells)
{
    if (localRDeltaT().size() != nCells) FatalErrorIn("localEulerDdtScheme", "the field '" + rDeltaTName_ + "' has another size than the mesh");
    return field_;
}
fv::CoEulerDdtScheme::CoEulerDdtScheme(const word& phiName, const word& rhoName, scalar maxCo)
    : phiName_(phiName), rhoName_(rhoName), maxCo_(maxCo), deltaT_(0), addr_(nullptr), deltaCoeffs_(nullptr), magSf_(nullptr), weights_(nullptr), phi_(nullptr),
      rhoOld_(nullptr)
{
    if (!(maxCo_ > 0)) FatalErrorIn("CoEulerDdtScheme", "maxCo = " + std::to_string(maxCo_) + " should be > 0");
}
fv::CoEulerDdtScheme fv::CoEulerDdtScheme::New(const std::string& scheme)
{
    const mi_ddt_local_scheme s = parseLocal(scheme, MI_DDT_CO_EULER, "CoEuler");
    return CoEulerDdtScheme(s.name, s.rho_name, s.max_co);
}
void fv::CoEulerDdtScheme::setMesh(const lduAddressing& a, const scalargpuField& deltaCoeffs, const scalargpuField& magSf, const scalargpuField& weights)
{
    addr_ = &a; deltaCoeffs_ = &deltaCoeffs; magSf_ = &magSf; weights_ = &weights;
}
void fv::CoEulerDdtScheme::bind(const word& phiName, const scalargpuField& phi, const word& rhoName, const scalargpuField* rhoOld)
{
    if (phiName != phiName_) FatalErrorIn("CoEulerDdtScheme", "the scheme reads the flux '" + phiName_ + "', not '" + phiName + "'");
    if (rhoOld && rhoName != rhoName_) FatalErrorIn("CoEulerDdtScheme", "the scheme reads the density '" + rhoName_ + "', not '" + rhoName + "'");
    phi_ = &phi; rhoOld_ = rhoOld;
}
void fv::CoEulerDdtScheme::addPatch(const fvPatchCells& cells, const scalargpuField& pDeltaCoeffs, const scalargpuField& pMagSf, const scalargpuField& pPhi,
                                    const scalargpuField* pRhoOld)
{
    patches_.push_back({&cells, &pDeltaCoeffs, &pMagSf, &pPhi, pRhoOld});
}
void fv::CoEulerDdtScheme::CorDeltaT(scalargpuField& rDeltaT) const
{
    if (!addr_ || !phi_) FatalErrorIn("CoEulerDdtScheme", "setMesh and bind('" + phiName_ + "', ...) come first");
    miCheck(mi_co_r_delta_t(addr_->handle(), deltaCoeffs_->data(), magSf_->data(), phi_->data(), rhoOld_ ? weights_->data() : nullptr,
                            rhoOld_ ? rhoOld_->data() : nullptr, deltaT_, maxCo_, rDeltaT.data()), "CoEulerDdtScheme::CorDeltaT");
    for (const patchIn& p : patches_) {
        if (p.cells->size() == 0) continue;
        if (rhoOld_ && !p.rhoOld) FatalErrorIn("CoEulerDdtScheme", "a mass flux needs the old density '" + rhoName_ + "' on every patch");
        scalargpuField x(p.cells->size());
        miCheck(mi_co_face_r_delta_t(miEngine::New().ctx, x.size(), p.deltaCoeffs->data(), p.magSf->data(), p.phi->data(), rhoOld_ ? p.rhoOld->data() : nullptr,
                                     deltaT_, maxCo_, x.data()), "CoEulerDdtScheme::CofrDeltaT");
        miCheck(mi_patch_max(p.cells->handle(), x.data(), rDeltaT.data()), "CoEulerDdtScheme::CorDeltaT");
    }
}
const scalargpuField* fv::CoEulerDdtScheme::rDeltaT(label nCells)
{
    if (!rDeltaT_ || rDeltaT_->size() != nCells) rDeltaT_.reset(new scalargpuField(nCells));
    CorDeltaT(*rDeltaT_);
    return rDeltaT_.get();
}
bool fv::boundedConvection(std::vector<std::string>& entry)
{
    if (entry.empty() || entry[0] != "bounded") return false;
    entry.erase(entry.begin());
    return true;
}
void fvm::assembleLocal(lduMatrix& M, scalargpuField* const* sources, const scalargpuField* rDeltaT, scalar rho, const scalargpuField& V,
                        const scalargpuField* const* psiOld, int nRhs, const scalargpuField* faceFlux, const scalargpuField* weights, const scalargpuField* deltaCoeffs,
                        const scalargpuField* gammaMagSf, const scalargpuField* divPhi, const linearUpwindCorrection* corr, const scalargpuField* su)
{
    const char* where = "fvm::assemble (steadyState | localEuler | CoEuler, bounded)";
    if (nRhs < 1 || nRhs > 3 || !sources || !psiOld) FatalErrorIn(where, "1 to 3 right-hand sides, " + std::to_string(nRhs) + " given");
    mi_fvm_terms t{};
    t.ddt = rDeltaT ? 1 : 0; t.rho_value = rho; t.vol_dev = V.data();
    t.div_flux_dev = faceFlux ? faceFlux->data() : nullptr; t.div_weights_dev = weights ? weights->data() : nullptr;
    t.lap_delta_coeffs_dev = deltaCoeffs ? deltaCoeffs->data() : nullptr; t.lap_gamma_magsf_dev = gammaMagSf ? gammaMagSf->data() : nullptr;
    const double* po[3]; double* so[3];
    for (int r = 0; r < nRhs; ++r) { po[r] = psiOld[r]->data(); so[r] = sources[r]->data(); }
    t.n_rhs = nRhs; t.psi_old_dev = po;
    const double* sd[1] = {su ? su->data() : nullptr}; const double sg[1] = {1.0};
    if (su) { t.n_su = 1; t.su_dev = sd; t.su_sign = sg; }
    mi_div_correction k{};
    if (corr) k = divCorrection(*corr, (std::size_t)nRhs);
    const mi_addr_t a = M.lduAddr().handle();
    double *lower = faceFlux ? M.lower().data() : nullptr, *upper = M.upper().data(), *diag = M.diag().data();
    if (!rDeltaT && !divPhi) {                        // steadyState with a plain convection scheme: the assembly without a time derivative
        miCheck(mi_fvm_assemble_corrected(a, &t, corr ? &k : nullptr, lower, upper, diag, so, nullptr), where);
        return;
    }
    const mi_fvm_local_terms loc{rDeltaT ? rDeltaT->data() : nullptr, divPhi ? divPhi->data() : nullptr};
    miCheck(mi_fvm_assemble_local(a, &t, &loc, corr ? &k : nullptr, lower, upper, diag, so, nullptr), where);
}
void fvm::assembleBounded(fvScalarMatrix& M, scalar rDeltaT, scalar rho, const scalargpuField& V, const scalargpuField& psiOld, const scalargpuField& faceFlux,
                          const scalargpuField* weights, const scalargpuField* deltaCoeffs, const scalargpuField* gammaMagSf, const scalargpuField& divPhi,
                          const linearUpwindCorrection* corr, const scalargpuField* su)
{
    mi_fvm_terms t{};
    t.ddt = 1; t.r_delta_t = rDeltaT; t.rho_value = rho; t.vol_dev = V.data();
    t.div_flux_dev = faceFlux.data(); t.div_weights_dev = weights ? weights->data() : nullptr;
    t.lap_delta_coeffs_dev = deltaCoeffs ? deltaCoeffs->data() : nullptr; t.lap_gamma_magsf_dev = gammaMagSf ? gammaMagSf->data() : nullptr;
    const double* po[1] = {psiOld.data()}; double* so[1] = {M.source().data()};
    t.n_rhs = 1; t.psi_old_dev = po;
    const double* sd[1] = {su ? su->data() : nullptr}; const double sg[1] = {1.0};
    if (su) { t.n_su = 1; t.su_dev = sd; t.su_sign = sg; }
    mi_div_correction k{};
    if (corr) k = divCorrection(*corr, 1);
    const mi_fvm_local_terms loc{nullptr, divPhi.data()};
    miCheck(mi_fvm_assemble_local(M.lduAddr().handle(), &t, &loc, corr ? &k : nullptr, M.lower().data(), M.upper().data(), M.diag().data(), so, nullptr),
            "fvm::assemble (bounded)");
}
namespace {
void ddtLocal(fvScalarMatrix& M, const scalargpuField* r, scalar rho, const scalargpuField& V, const scalargpuField& psiOld)
{
    if (!r) {                                         // steadyState: the empty matrix
        miDeviceZero(M.diag().data(), sizeof(scalar) * (std::size_t)M.diag().size());
        miDeviceZero(M.source().data(), sizeof(scalar) * (std::size_t)M.source().size());
        return;
    }
    miCheck(mi_fvm_ddt_local(miEngine::New().ctx, V.size(), r->data(), rho, nullptr, nullptr, V.data(), psiOld.data(), M.diag().data(), M.source().data()),
            "fvm::ddt (localEuler | CoEuler)");
}
void fvcDdtLocal(scalargpuField& out, const scalargpuField* r, const scalargpuField& vf, const scalargpuField& vfOld)
{
    if (!r) { miDeviceZero(out.data(), sizeof(scalar) * (std::size_t)out.size()); return; }
    miCheck(mi_fvc_ddt_local(miEngine::New().ctx, vf.size(), r->data(), 1.0, nullptr, nullptr, vf.data(), vfOld.data(), out.data()), "fvc::ddt (localEuler | CoEuler)");
}
void ddtCorrLocal(scalargpuField& out, const lduAddressing& a, const scalargpuField* r, const scalargpuField& weights, const vectorgpuField& Sf,
                  const vectorgpuField& Uold, const scalargpuField& phiOld)
{
    if (!r) { miDeviceZero(out.data(), sizeof(scalar) * (std::size_t)out.size()); return; }
    miCheck(mi_ddt_phi_corr_local(a.handle(), r->data(), weights.data(), Sf.component(0).data(), Sf.component(1).data(), Sf.component(2).data(),
                                  Uold.component(0).data(), Uold.component(1).data(), Uold.component(2).data(), phiOld.data(), out.data()),
            "fvc::ddtCorr (localEuler | CoEuler)");
}
}
void fvm::ddt(fvScalarMatrix& M, fv::steadyStateDdtScheme& s, scalar rho, const scalargpuField& V, const scalargpuField& psiOld) { ddtLocal(M, s.rDeltaT(V.size()), rho, V, psiOld); }
void fvm::ddt(fvScalarMatrix& M, fv::localEulerDdtScheme& s, scalar rho, const scalargpuField& V, const scalargpuField& psiOld) { ddtLocal(M, s.rDeltaT(V.size()), rho, V, psiOld); }
void fvm::ddt(fvScalarMatrix& M, fv::CoEulerDdtScheme& s, scalar rho, const scalargpuField& V, const scalargpuField& psiOld) { ddtLocal(M, s.rDeltaT(V.size()), rho, V, psiOld); }
void fvc::ddt(scalargpuField& out, fv::steadyStateDdtScheme& s, const scalargpuField& vf, const scalargpuField& vfOld) { fvcDdtLocal(out, s.rDeltaT(vf.size()), vf, vfOld); }
void fvc::ddt(scalargpuField& out, fv::localEulerDdtScheme& s, const scalargpuField& vf, const scalargpuField& vfOld) { fvcDdtLocal(out, s.rDeltaT(vf.size()), vf, vfOld); }
void fvc::ddt(scalargpuField& out, fv::CoEulerDdtScheme& s, const scalargpuField& vf, const scalargpuField& vfOld) { fvcDdtLocal(out, s.rDeltaT(vf.size()), vf, vfOld); }
void fvc::ddtCorr(scalargpuField& out, const lduAddressing& a, fv::steadyStateDdtScheme& s, const scalargpuField& weights, const vectorgpuField& Sf,
                  const vectorgpuField& Uold, const scalargpuField& phiOld)
{
    ddtCorrLocal(out, a, s.rDeltaT(Uold.size()), weights, Sf, Uold, phiOld);
}
void fvc::ddtCorr(scalargpuField& out, const lduAddressing& a, fv::localEulerDdtScheme& s, const scalargpuField& weights, const vectorgpuField& Sf,
                  const vectorgpuField& Uold, const scalargpuField& phiOld)
{
    ddtCorrLocal(out, a, s.rDeltaT(Uold.size()), weights, Sf, Uold, phiOld);
}
void fvc::ddtCorr(scalargpuField& out, const lduAddressing& a, fv::CoEulerDdtScheme& s, const scalargpuField& weights, const vectorgpuField& Sf,
                  const vectorgpuField& Uold, const scalargpuField& phiOld)
{
    ddtCorrLocal(out, a, s.rDeltaT(Uold.size()), weights, Sf, Uold, phiOld);
}
void fvc::divBounded(scalargpuField& out, const lduAddressing& a, const scalargpuField& faceFlux, const scalargpuField* weights, const scalargpuField& vf,
                     const scalargpuField& V, const scalargpuField& divPhi)
{
    scalargpuField face(faceFlux.size());
    miCheck(mi_fvc_div(a.handle(), faceFlux.data(), weights ? weights->data() : nullptr, vf.data(), V.data(), face.data(), out.data()), "fvc::div (bounded)");
    fieldSubMul(out, divPhi, vf);                     // - (divPhi*vf): the product rounded first
}

// ---- hePsiThermo / heRhoThermo ---------------------------------------------------------------------------------------------------------------
hePsiThermo::hePsiThermo(const lduAddressing& addr, const gradBoundary& boundary, const std::vector<label>& patchSizes,
                         const std::vector<patchType>& TPatchTypes, const mi_thermo_model& model, const scalargpuField& p, const scalargpuField& bp,
                         const scalargpuField& T, const scalargpuField& bT, bool rhoThermo)
    : addr_(addr), boundary_(boundary), model_(model), patchSizes_(patchSizes), rhoForm_(rhoThermo ? 1 : 2), p_(p), bp_(bp), T_(T), bT_(bT)
{
    if (patchSizes.size() != TPatchTypes.size()) FatalErrorIn("hePsiThermo::hePsiThermo", "one type per patch");
    label nb = 0;
    for (std::size_t i = 0; i < patchSizes.size(); ++i) { kinds_.push_back((int32_t)TPatchTypes[i]); nb += patchSizes[i]; }
    if (p.size() != T.size() || bp.size() != nb || bT.size() != nb) FatalErrorIn("hePsiThermo::hePsiThermo", "field sizes do not match the mesh");
    const std::vector<scalar> seed((std::size_t)nb, std::numeric_limits<scalar>::quiet_NaN());
    he_ = scalargpuField(T.size()); psi_ = scalargpuField(T.size()); mu_ = scalargpuField(T.size()); alpha_ = scalargpuField(T.size());
    rho_ = scalargpuField(T.size());
    bhe_ = seed; bpsi_ = seed; bmu_ = seed; balpha_ = seed; brho_ = seed;
    init();
    calculate();
}
void hePsiThermo::init()
{
    const mi_ctx_t ctx = miEngine::New().ctx;
    miCheck(mi_thermo_he(ctx, &model_, T_.size(), p_.data(), T_.data(), he_.data()), "heThermo::init");
    label off = 0;
    for (std::size_t i = 0; i < patchSizes_.size(); ++i) {                // he(p, T, patchi) on the patch's slice
        if (kinds_[i] != empty && patchSizes_[i] > 0)
            miCheck(mi_thermo_he(ctx, &model_, patchSizes_[i], bp_.data() + off, bT_.data() + off, bhe_.data() + off), "heThermo::init");
        off += patchSizes_[i];
    }
}
void hePsiThermo::correct() { calculate(); }
void hePsiThermo::calculate()
{
    const mi_ctx_t ctx = miEngine::New().ctx;
    miCheck(mi_thermo_calculate(ctx, &model_, rhoForm_, T_.size(), he_.data(), p_.data(), T_.data(), T_.data(), psi_.data(), mu_.data(), alpha_.data(),
                                rho_.data(), nullptr), "hePsiThermo::calculate");
    miCheck(mi_thermo_calculate_boundary(addr_.handle(), boundary_.handle(), &model_, kinds_.data(), rhoForm_, bhe_.data(), bp_.data(), bT_.data(),
                                         bT_.data(), bpsi_.data(), bmu_.data(), balpha_.data(), brho_.data()), "hePsiThermo::calculate");
}
static void thermoProperty(const mi_thermo_model& m, int kind, const scalargpuField& p, const scalargpuField& T, scalargpuField& out)
{
    if (out.size() != T.size()) FatalErrorIn("heThermo::Cp", "field sizes do not match");
    miCheck(mi_thermo_property(miEngine::New().ctx, &m, kind, T.size(), p.data(), T.data(), out.data()), "heThermo::Cp");
}
void hePsiThermo::Cp(scalargpuField& cells, scalargpuField& boundary) const
{
    thermoProperty(model_, MI_THERMO_CP, p_, T_, cells); thermoProperty(model_, MI_THERMO_CP, bp_, bT_, boundary);
}
void hePsiThermo::Cv(scalargpuField& cells, scalargpuField& boundary) const
{
    thermoProperty(model_, MI_THERMO_CV, p_, T_, cells); thermoProperty(model_, MI_THERMO_CV, bp_, bT_, boundary);
}

// ---- rhoCentralFoam's flux evaluation (rhoCentralFoam.C:60-185) ------------------------------------------------------------------------
centralFluxes::centralFluxes(const lduAddressing& addr, const std::vector<labelList>& patchFaceCells, const word& fluxScheme, const word& reconstructRho,
                             const word& reconstructU, const word& reconstructT, const geometry& g)
    : addr_(addr), g_(g), rPsi_(addr.size()), c_(addr.size()), brPsi_(g.bMagSf.size()), bc_(g.bMagSf.size()), ssf_(g.magSf.size()),
      gradRho_(addr.size()), gradRPsi_(addr.size()), gradE_(addr.size()), gradC_(addr.size()), gradRhoU0_(addr.size()), gradRhoU1_(addr.size()),
      gradRhoU2_(addr.size()), phi_(g.magSf.size()), phiEp_(g.magSf.size()), amaxSf_(g.magSf.size()), bphi_(g.bMagSf.size()), bphiEp_(g.bMagSf.size()),
      bamaxSf_(g.bMagSf.size()), phiUp_(g.magSf.size()), bphiUp_(g.bMagSf.size())
{
    miCheck(mi_central_scheme_parse(fluxScheme.c_str(), reconstructRho.c_str(), reconstructU.c_str(), reconstructT.c_str(), &scheme_), "readFluxScheme.H");
    if (!scheme_.U.vector_form) FatalErrorIn("centralFluxes::centralFluxes", "reconstruct(U) must be a V scheme here: a scalar scheme limits on magSqr(rhoU), the caller's field");
    label nb = 0;
    for (const labelList& fc : patchFaceCells) { patches_.emplace_back(new fvPatchCells(addr.size(), fc)); nb += (label)fc.size(); }
    if (nb != g.bMagSf.size() || g.bSf.size() != nb || g.bDeltaCoeffs.size() != nb) FatalErrorIn("centralFluxes::centralFluxes", "the boundary geometry does not match the patches");
}
// fvc::grad, Gauss linear: the boundary faces add Sf_b*vf_b to their cells patch by patch before the division by V (gaussGrad.C:143-250)
void centralFluxes::grad(vectorgpuField& g, const scalargpuField& vf, const scalargpuField& bvf)
{
    const mi_ctx_t ctx = miEngine::New().ctx;
    miCheck(mi_face_interpolate(addr_.handle(), g_.weights.data(), vf.data(), ssf_.data()), "fvc::interpolate");
    miCheck(mi_gauss_grad(addr_.handle(), g_.Sf.c[0].data(), g_.Sf.c[1].data(), g_.Sf.c[2].data(), ssf_.data(), nullptr, g.c[0].data(), g.c[1].data(),
                          g.c[2].data()), "fvc::grad");
    for (direction d = 0; d < 3; ++d) {
        label off = 0;
        for (const auto& p : patches_) {
            if (p->size()) miCheck(mi_patch_add_product(p->handle(), g_.bSf.c[d].data() + off, bvf.data() + off, g.c[d].data(), 0), "fvc::grad");
            off += p->size();
        }
        miCheck(mi_vec_div(ctx, g.size(), g.c[d].data(), g_.V.data(), g.c[d].data()), "fvc::grad");
    }
}
void centralFluxes::update(const volFields& v, const volFields& b)
{
    const mi_ctx_t ctx = miEngine::New().ctx;
    const label n = addr_.size(), nb = g_.bMagSf.size();
    miCheck(mi_central_sound_speed(ctx, n, v.Cp.data(), v.Cv.data(), v.psi.data(), rPsi_.data(), c_.data()), "rhoCentralFoam.C:84,116");
    if (nb) miCheck(mi_central_sound_speed(ctx, nb, b.Cp.data(), b.Cv.data(), b.psi.data(), brPsi_.data(), bc_.data()), "rhoCentralFoam.C:84,116");
    grad(gradRho_, v.rho, b.rho); grad(gradRPsi_, rPsi_, brPsi_); grad(gradE_, v.e, b.e); grad(gradC_, c_, bc_);
    vectorgpuField* const gU[3] = {&gradRhoU0_, &gradRhoU1_, &gradRhoU2_};
    for (direction d = 0; d < 3; ++d) grad(*gU[d], v.rhoU.c[d], b.rhoU.c[d]);
    mi_central_cells cells{};
    cells.rho_dev = v.rho.data(); cells.rpsi_dev = rPsi_.data(); cells.e_dev = v.e.data(); cells.c_dev = c_.data();
    for (int k = 0; k < 3; ++k) {
        cells.rhou_dev[k] = v.rhoU.c[k].data(); cells.grad_rho_dev[k] = gradRho_.c[k].data(); cells.grad_rpsi_dev[k] = gradRPsi_.c[k].data();
        cells.grad_e_dev[k] = gradE_.c[k].data(); cells.grad_c_dev[k] = gradC_.c[k].data();
        for (int j = 0; j < 3; ++j) cells.grad_rhou_dev[3 * j + k] = gU[j]->c[k].data();
    }
    mi_central_out out{};
    out.phi_out_dev = phi_.data(); out.phiep_out_dev = phiEp_.data(); out.amaxsf_out_dev = amaxSf_.data();
    for (int k = 0; k < 3; ++k) out.phiup_out_dev[k] = phiUp_.c[k].data();
    const double* const sf[3] = {g_.Sf.c[0].data(), g_.Sf.c[1].data(), g_.Sf.c[2].data()};
    const double* const cc[3] = {g_.C.c[0].data(), g_.C.c[1].data(), g_.C.c[2].data()};
    miCheck(mi_central_flux(addr_.handle(), &scheme_, g_.weights.data(), sf, g_.magSf.data(), &cells, cc, &out), "rhoCentralFoam.C:62-185");
    label off = 0;
    for (const auto& p : patches_) {                          // the boundary value is the face value of both directions
        mi_central_cells vals{};
        vals.rho_dev = b.rho.data() + off; vals.rpsi_dev = brPsi_.data() + off; vals.e_dev = b.e.data() + off; vals.c_dev = bc_.data() + off;
        mi_central_out po{};
        po.phi_out_dev = bphi_.data() + off; po.phiep_out_dev = bphiEp_.data() + off; po.amaxsf_out_dev = bamaxSf_.data() + off;
        const double* psf[3];
        for (int k = 0; k < 3; ++k) { vals.rhou_dev[k] = b.rhoU.c[k].data() + off; po.phiup_out_dev[k] = bphiUp_.c[k].data() + off; psf[k] = g_.bSf.c[k].data() + off; }
        miCheck(mi_patch_central_flux(p->handle(), &scheme_, nullptr, psf, g_.bMagSf.data() + off, &vals, nullptr, nullptr, &po), "rhoCentralFoam.C:62-185");
        off += p->size();
    }
}
void centralFluxes::CourantNo(scalar deltaT, scalar sumMagSf, scalar& CoNum, scalar& meanCoNum) const
{
    scalar mx = 0.0, sm = 0.0;
    miCheck(mi_central_courant(addr_.handle(), g_.deltaCoeffs.data(), g_.magSf.data(), amaxSf_.data(), g_.bMagSf.size(), g_.bDeltaCoeffs.data(),
                               g_.bMagSf.data(), bamaxSf_.data(), &mx, &sm), "compressibleCourantNo.H");
    CoNum = 0.5 * mx * deltaT;
    meanCoNum = 0.5 * (sm / sumMagSf) * deltaT;
}
void centralFluxes::solveDdtDiv(scalargpuField& vf, scalar rDeltaT, const scalargpuField& flux, const scalargpuField& bflux)
{
    const mi_ctx_t ctx = miEngine::New().ctx;
    const label n = addr_.size();
    scalargpuField diag(n), source(n), dv(n);
    miCheck(mi_fvm_ddt_euler(ctx, n, rDeltaT, 1.0, g_.V.data(), vf.data(), diag.data(), source.data()), "fvm::ddt");
    miCheck(mi_surface_integrate(addr_.handle(), flux.data(), nullptr, dv.data()), "fvc::div");
    label off = 0;
    for (const auto& p : patches_) {
        if (p->size()) miCheck(mi_patch_add(p->handle(), bflux.data() + off, dv.data(), 0), "fvc::div");
        off += p->size();
    }
    miCheck(mi_vec_div(ctx, n, dv.data(), g_.V.data(), dv.data()), "fvc::div");
    miCheck(mi_vec_submul(ctx, n, g_.V.data(), dv.data(), source.data()), "fvMatrix + volField");
    miCheck(mi_vec_div(ctx, n, source.data(), diag.data(), vf.data()), "fvMatrix::solve");
}

} // namespace Foam
