// row_entry.inc -- what a row-pass entry does on the host before it launches (included by engine.hip after assembly.inc; DESIGN 3.5): the
// row tables every row kernel of the files below walks, the launch that picks the 256 / 512 / 1024 instantiation on the gradient's plan,
// the members and checks every handle over an addressing and a boundary shares, and the checks of a call's arrays.  A new row pass starts
// here: a struct with a RowTables r, a handle derived from RowHandle, the primitives below in the order its faults are to be reported.
namespace mi {

// the caller-order row tables, the block mapping and the per-cell boundary face lists; cap is set by row_launch_bs
struct RowTables {
    const int32_t *os, *ls, *losort, *blockStart, *lo, *up;
    const int32_t *bStart, *bFace;                    // indices into the patch-ordered boundary faces, or NULL: no boundary faces
    int n, cap, xcd;
};

} // namespace mi

// the boundary of a row pass: every boundary face's cell, in patch order, as a per-cell list; the face kinds of the limited gradient read
// only the coupled and fixesValue patches (faceLimitedGrads.C:119-163), so they get a list of their own
struct mi_grad_boundary_s {
    mi_ctx_s* ctx = nullptr;
    mi_addr_s* addr = nullptr;
    int32_t nCells = 0, nFaces = 0, nLimited = 0;
    DevBuf<int32_t> allStart, all, limStart, lim;
    std::vector<int32_t> patchSizes, patchKinds;      // the patches as given (least_squares.inc marks the coupled faces from them)
};

// what every handle over an addressing and its boundary opens with
struct RowHandle {
    mi_ctx_s* ctx = nullptr;
    mi_addr_s* addr = nullptr;
    mi_grad_boundary_s* boundary = nullptr;
    int32_t nCells = 0, nFaces = 0, nBFaces = 0;
};

namespace {
// ---- a call's arrays ---------------------------------------------------------------------------------------------------------------------
int arrays_present(const std::string& who, const double* const* in, int n)
{
    for (int i = 0; i < n; ++i) if (!in[i]) return fail(MI_ERR_ARG, who + ": input arrays missing");
    return MI_OK;
}
// every output present, not among the inputs and not twice
int outputs_distinct(const std::string& who, const double* const* in, int nIn, double* const* out, int nOut)
{
    for (int o = 0; o < nOut; ++o) {
        if (!out[o]) return fail(MI_ERR_ARG, who + ": output arrays missing");
        for (int i = 0; i < nIn; ++i) if (out[o] == in[i]) return fail(MI_ERR_ARG, who + ": an output must not alias an input");
        for (int q = 0; q < o; ++q) if (out[o] == out[q]) return fail(MI_ERR_ARG, who + ": the outputs must differ");
    }
    return MI_OK;
}
int arrays_aligned8(const std::string& who, const void* const* p, int n)
{
    for (int i = 0; i < n; ++i) if (!al8(p[i])) return fail(MI_ERR_ARG, who + ": arrays must be aligned to 8 bytes");
    return MI_OK;
}
bool all_aligned16(const double* const* in, int nIn, double* const* out, int nOut)
{
    bool v = true;
    for (int i = 0; i < nIn; ++i) v = v && al16(in[i]);
    for (int i = 0; i < nOut; ++i) v = v && al16(out[i]);
    return v;
}

// ---- the row tables and the launch (after ensure_caller_tables) ----------------------------------------------------------------------------
RowTables row_tables(mi_addr_s* a, const int32_t* bStart, const int32_t* bFace)
{
    RowTables r{};
    r.os = a->ownerStartC.p; r.ls = a->losortStartC.p; r.losort = a->losortC.p; r.lo = a->lowerAddr.p; r.up = a->upperAddr.p;
    r.blockStart = a->rowPlan[1].tiles ? a->tileCellStart.p : nullptr;
    r.bStart = bStart; r.bFace = bFace;
    r.n = a->L.nCells; r.xcd = a->ctx->xcdRows;
    return r;
}
RowTables row_tables(mi_addr_s* a, const mi_grad_boundary_s* b)
{
    const bool faces = b && b->nFaces > 0;
    return row_tables(a, faces ? b->allStart.p : nullptr, faces ? b->all.p : nullptr);
}
// a row pass of `arrays` staged face arrays on the gradient's plan, its argument q holding a RowTables r: the instantiation of the plan's
// block size, row_cap's doubles of LDS for each array
template <class K, class A>
int row_launch_bs(mi_addr_s* a, int arrays, K k256, K k512, K k1024, A& q)
{
    const mi_addr_s::RowPlan& rp = a->rowPlan[1];
    q.r.cap = row_cap(rp, arrays);
    return row_launch(a, rp, rp.bs == 256 ? k256 : rp.bs == 512 ? k512 : k1024, q, (size_t)arrays * q.r.cap * sizeof(double));
}
#define ROW_BS(K, ...) K<256, ##__VA_ARGS__>, K<512, ##__VA_ARGS__>, K<1024, ##__VA_ARGS__>

// ---- the handles -------------------------------------------------------------------------------------------------------------------------
int boundary_matches(const std::string& who, const mi_addr_s* a, const mi_grad_boundary_s* b)
{
    if (b && (b->addr != a || b->nCells != a->L.nCells)) return fail(MI_ERR_ARG, who + ": the boundary was built for another addressing");
    return MI_OK;
}
// the opening of a create: the arguments, then the shared members of h.  Host work only: a create tests its own arrays next and only then
// selects the device and (where its kernels walk them) builds the caller-order tables, so the order of its refusals is its own
int row_handle_open(const std::string& who, mi_addr_s* a, mi_grad_boundary_s* b, const void* out, RowHandle& h)
{
    if (!a || !out) return fail(MI_ERR_ARG, who + ": bad argument");
    MICHK(boundary_matches(who, a, b));
    h.ctx = a->ctx; h.addr = a; h.boundary = b; h.nCells = a->L.nCells; h.nFaces = a->L.nFaces; h.nBFaces = b ? b->nFaces : 0;
    return MI_OK;
}
// the opening of a use: the handle still describes its addressing and its boundary.  The boundary's face count is compared too, as
// fvc::average's check always did: it never changes after the boundary's creation, so this refuses nothing that the looser forms let pass
int row_handle_check(const std::string& who, const RowHandle* h, const char* subject = "the handle was")
{
    if (!h) return fail(MI_ERR_ARG, who + ": bad argument");
    const mi_addr_s* a = h->addr;
    if (h->nCells != a->L.nCells || h->nFaces != a->L.nFaces || (h->boundary && (h->boundary->addr != a || h->boundary->nFaces != h->nBFaces)))
        return fail(MI_ERR_ARG, who + ": " + subject + " built for another addressing");
    return MI_OK;
}
} // namespace
