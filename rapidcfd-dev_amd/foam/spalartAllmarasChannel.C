// spalartAllmarasChannel -- a test driver, not an application: it runs one of the mirror's Spalart-Allmaras classes
// (incompressible::RASModels::SpalartAllmaras, LESModels::SpalartAllmaras, SpalartAllmarasDDES, SpalartAllmarasIDDES: its constructor and
// `steps` calls of correct()) on a case that tests/test_spalart_allmaras.py writes as raw arrays into a directory, and writes nuTilda and
// nut / nuSgs with their boundary values back after the constructor (step 0) and after every correct().  The flow (U, grad(U) with its
// boundary values, phi) is frozen; the wall distance (yCell per cell, y per boundary face), delta and hmax (cells and boundary faces) and the
// face area vectors (Sf, bSf) are inputs.
//   <dir>/meta.txt   model n nf steps rDeltaT nu nuTildaRelax nPatches, then per patch: size type (0 fixedValue, 1 zeroGradient, 2 wall);
//                    model: RAS | DES | DDES | IDDES
//   <dir>/<name>.bin float64 or int32, native byte order
#include "miFoam.H"

#include <cstdio>
#include <fstream>

using namespace Foam;

template <class T>
static std::vector<T> readRaw(const std::string& dir, const std::string& name, std::size_t count)
{
    std::vector<T> v(count);
    std::ifstream f(dir + "/" + name + ".bin", std::ios::binary);
    if (!f || (count && !f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T))))) FatalErrorIn("spalartAllmarasChannel", "cannot read " + name);
    return v;
}
static void writeRaw(const std::string& dir, const std::string& name, const scalargpuField& x)
{
    const std::vector<scalar> h = x.asHost();
    std::ofstream f(dir + "/" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(h.data()), (std::streamsize)(h.size() * sizeof(scalar)));
    if (!f) FatalErrorIn("spalartAllmarasChannel", "cannot write " + name);
}
static vectorgpuField readVector(const std::string& dir, const std::string& name, std::size_t count)
{
    vectorgpuField v((label)count);
    for (int d = 0; d < 3; ++d) v.c[d] = readRaw<scalar>(dir, name + std::to_string(d), count);
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: spalartAllmarasChannel <dir>\n"); return 2; }
    try {
        typedef incompressible::SpalartAllmarasBase model;
        const std::string dir = argv[1];
        std::ifstream meta(dir + "/meta.txt");
        std::string which;
        label n = 0, nf = 0, steps = 0, nPatches = 0;
        scalar rDeltaT = 0, nu = 0, relax = 1;
        meta >> which >> n >> nf >> steps >> rDeltaT >> nu >> relax >> nPatches;
        std::vector<label> sizes((std::size_t)nPatches);
        std::vector<model::patchType> types;
        label nb = 0;
        for (label p = 0; p < nPatches; ++p) { int t = 0; meta >> sizes[(std::size_t)p] >> t; types.push_back((model::patchType)t); nb += sizes[(std::size_t)p]; }
        if (!meta) FatalErrorIn("spalartAllmarasChannel", "bad meta.txt");
        const labelList lower = readRaw<label>(dir, "lower", (std::size_t)nf), upper = readRaw<label>(dir, "upper", (std::size_t)nf);
        const labelList allCells = readRaw<label>(dir, "faceCells", (std::size_t)nb);
        std::vector<labelList> faceCells;
        std::vector<gradBoundary::patchKind> kinds;
        label off = 0;
        for (label p = 0; p < nPatches; ++p) {
            faceCells.emplace_back(allCells.begin() + off, allCells.begin() + off + sizes[(std::size_t)p]);
            kinds.push_back(types[(std::size_t)p] == model::fixedValue ? gradBoundary::fixesValue : gradBoundary::other);
            off += sizes[(std::size_t)p];
        }
        lduAddressing addr(n, lower, upper);
        gradBoundary boundary(addr, faceCells, kinds);
        auto cellField = [&](const char* name) { return scalargpuField(readRaw<scalar>(dir, name, (std::size_t)n)); };
        auto faceField = [&](const char* name) { return scalargpuField(readRaw<scalar>(dir, name, (std::size_t)nf)); };
        auto patchField = [&](const char* name) { return scalargpuField(readRaw<scalar>(dir, name, (std::size_t)nb)); };
        const scalargpuField weights = faceField("weights"), deltaCoeffs = faceField("deltaCoeffs"), magSf = faceField("magSf"), V = cellField("V");
        const scalargpuField bMagSf = patchField("bMagSf"), bDeltaCoeffs = patchField("bDeltaCoeffs"), y = cellField("yCell"), bY = patchField("y");
        const scalargpuField delta = cellField("delta"), bDelta = patchField("bDelta"), hmax = cellField("hmax"), bHmax = patchField("bHmax");
        const vectorgpuField Sf = readVector(dir, "Sf", (std::size_t)nf), bSf = readVector(dir, "bSf", (std::size_t)nb);
        const scalargpuField phi = faceField("phi"), bPhi = patchField("bPhi");
        const vectorgpuField U = readVector(dir, "U", (std::size_t)n), bU = readVector(dir, "bU", (std::size_t)nb);
        const vectorgpuField g0 = readVector(dir, "gradU0_", (std::size_t)n), g1 = readVector(dir, "gradU1_", (std::size_t)n), g2 = readVector(dir, "gradU2_", (std::size_t)n);
        const vectorgpuField* gradU[3] = {&g0, &g1, &g2};
        const vectorgpuField b0 = readVector(dir, "bgradU0_", (std::size_t)nb), b1 = readVector(dir, "bgradU1_", (std::size_t)nb), b2 = readVector(dir, "bgradU2_", (std::size_t)nb);
        const vectorgpuField* bGradU[3] = {&b0, &b1, &b2};
        averageData average(addr, &boundary, magSf, &bMagSf);
        const model::meshData mesh = {&addr, &boundary, &average, faceCells, types, &weights, &deltaCoeffs, &magSf, &V, &bMagSf, &bDeltaCoeffs, &y, &bY, &Sf, &bSf,
                                      &delta, &bDelta, &hmax, &bHmax};
        const model::flowData flow = {&U, &bU, gradU, bGradU, &phi, &bPhi, nullptr};
        const scalargpuField nuTilda0 = cellField("nuTilda"), bnuTilda0 = patchField("bnuTilda");
        std::unique_ptr<model> turbulence;
        const scalargpuField* nut = nullptr; const scalargpuField* bnut = nullptr;
        if (which == "RAS") {
            auto* m = new incompressible::RASModels::SpalartAllmaras(mesh, flow, nu, nuTilda0, bnuTilda0);
            turbulence.reset(m); nut = &m->nut(); bnut = &m->nutBoundary();
        } else {
            incompressible::LESModels::SpalartAllmaras* m = nullptr;
            if (which == "DES") m = new incompressible::LESModels::SpalartAllmaras(mesh, flow, nu, nuTilda0, bnuTilda0);
            else if (which == "DDES") m = new incompressible::LESModels::SpalartAllmarasDDES(mesh, flow, nu, nuTilda0, bnuTilda0);
            else if (which == "IDDES") m = new incompressible::LESModels::SpalartAllmarasIDDES(mesh, flow, nu, nuTilda0, bnuTilda0);
            else FatalErrorIn("spalartAllmarasChannel", "unknown model " + which);
            turbulence.reset(m); nut = &m->nuSgs(); bnut = &m->nuSgsBoundary();
            scalargpuField s(n), d(n);                      // the virtuals through the base class: written for the test
            m->S(s, flow); m->dTilda(d, flow);
            writeRaw(dir, "S_0", s); writeRaw(dir, "dTilda_0", d);
        }
        const dictionary controls({{"solver", "PBiCG"}, {"preconditioner", "diagonal"}, {"tolerance", "1e-10"}, {"relTol", "0"}, {"maxIter", "300"}});
        for (label step = 0; step <= steps; ++step) {
            if (step > 0) turbulence->correct(flow, rDeltaT, controls, relax);
            const std::string s = std::to_string(step);
            writeRaw(dir, "nuTilda_" + s, turbulence->nuTilda()); writeRaw(dir, "bnuTilda_" + s, turbulence->nuTildaBoundary());
            writeRaw(dir, "nut_" + s, *nut); writeRaw(dir, "bnut_" + s, *bnut);
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
