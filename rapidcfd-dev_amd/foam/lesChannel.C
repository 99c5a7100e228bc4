// lesChannel -- a test driver, not an application: it runs one of the mirror's incompressible::LESModels (Smagorinsky, oneEqEddy, dynOneEqEddy:
// its constructor and `steps` calls of correct()) on a case that tests/test_les.py writes as raw arrays into a directory, and writes k and
// nuSgs with their boundary values back after the constructor (step 0) and after every correct().  The flow is given per stage: stage 0 is
// what the constructor sees, stage s what the s-th correct() sees.
//   <dir>/meta.txt   model n nf steps rDeltaT nu kRelax nPatches, then per patch: size type (0 fixedValue, 1 zeroGradient)
//   <dir>/<name>.bin float64 or int32, native byte order; s<stage>_U<d>, s<stage>_bU<d>, s<stage>_gradU<j>_<d>, s<stage>_bGradU<j>_<d>
#include "miFoam.H"

#include <cstdio>
#include <fstream>

using namespace Foam;

template <class T>
static std::vector<T> readRaw(const std::string& dir, const std::string& name, std::size_t count)
{
    std::vector<T> v(count);
    std::ifstream f(dir + "/" + name + ".bin", std::ios::binary);
    if (!f || (count && !f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T))))) FatalErrorIn("lesChannel", "cannot read " + name);
    return v;
}
static void writeRaw(const std::string& dir, const std::string& name, const scalargpuField& x)
{
    const std::vector<scalar> h = x.asHost();
    std::ofstream f(dir + "/" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(h.data()), (std::streamsize)(h.size() * sizeof(scalar)));
    if (!f) FatalErrorIn("lesChannel", "cannot write " + name);
}
static vectorgpuField readVector(const std::string& dir, const std::string& name, std::size_t count)
{
    vectorgpuField v((label)count);
    for (int d = 0; d < 3; ++d) v.c[d] = readRaw<scalar>(dir, name + std::to_string(d), count);
    return v;
}
// the flow of one stage
struct stage
{
    vectorgpuField U, bU, g0, g1, g2, b0, b1, b2;
    const vectorgpuField* gradU[3];
    const vectorgpuField* bGradU[3];
    stage(const std::string& dir, const std::string& s, std::size_t n, std::size_t nb)
        : U(readVector(dir, s + "U", n)), bU(readVector(dir, s + "bU", nb)), g0(readVector(dir, s + "gradU0_", n)), g1(readVector(dir, s + "gradU1_", n)),
          g2(readVector(dir, s + "gradU2_", n)), b0(readVector(dir, s + "bGradU0_", nb)), b1(readVector(dir, s + "bGradU1_", nb)),
          b2(readVector(dir, s + "bGradU2_", nb)), gradU{&g0, &g1, &g2}, bGradU{&b0, &b1, &b2} {}
};

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: lesChannel <dir>\n"); return 2; }
    try {
        typedef incompressible::LESModels::GenEddyVisc model;
        const std::string dir = argv[1];
        std::ifstream meta(dir + "/meta.txt");
        std::string name;
        label n = 0, nf = 0, steps = 0, nPatches = 0;
        scalar rDeltaT = 0, nu = 0, kRelax = 1;
        meta >> name >> n >> nf >> steps >> rDeltaT >> nu >> kRelax >> nPatches;
        std::vector<label> sizes((std::size_t)nPatches);
        std::vector<model::patchType> types;
        label nb = 0;
        for (label p = 0; p < nPatches; ++p) { int t = 0; meta >> sizes[(std::size_t)p] >> t; types.push_back((model::patchType)t); nb += sizes[(std::size_t)p]; }
        if (!meta) FatalErrorIn("lesChannel", "bad meta.txt");
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
        auto cellField = [&](const char* f) { return scalargpuField(readRaw<scalar>(dir, f, (std::size_t)n)); };
        auto faceField = [&](const char* f) { return scalargpuField(readRaw<scalar>(dir, f, (std::size_t)nf)); };
        auto patchField = [&](const char* f) { return scalargpuField(readRaw<scalar>(dir, f, (std::size_t)nb)); };
        const scalargpuField weights = faceField("weights"), deltaCoeffs = faceField("deltaCoeffs"), magSf = faceField("magSf"), V = cellField("V");
        const scalargpuField bMagSf = patchField("bMagSf"), bDeltaCoeffs = patchField("bDeltaCoeffs");
        const scalargpuField phi = faceField("phi"), bPhi = patchField("bPhi");
        averageData average(addr, &boundary, magSf, &bMagSf);
        const model::meshData mesh = {&addr, &boundary, &average, faceCells, types, &weights, &deltaCoeffs, &magSf, &V, &bMagSf, &bDeltaCoeffs};
        std::vector<std::unique_ptr<stage>> stages;
        for (label s = 0; s <= steps; ++s) stages.emplace_back(new stage(dir, "s" + std::to_string(s) + "_", (std::size_t)n, (std::size_t)nb));
        auto flowOf = [&](label s) { const stage& g = *stages[(std::size_t)s]; return model::flowData{&g.U, &g.bU, g.gradU, g.bGradU, &phi, &bPhi, nullptr}; };
        std::unique_ptr<model> turbulence;
        if (name == "Smagorinsky") turbulence.reset(new incompressible::LESModels::Smagorinsky(mesh, flowOf(0), nu));
        else if (name == "oneEqEddy") turbulence.reset(new incompressible::LESModels::oneEqEddy(mesh, nu, cellField("k"), patchField("bk")));
        else if (name == "dynOneEqEddy") turbulence.reset(new incompressible::LESModels::dynOneEqEddy(mesh, flowOf(0), nu, cellField("k"), patchField("bk")));
        else FatalErrorIn("lesChannel", "unknown model " + name);
        const dictionary controls({{"solver", "PBiCG"}, {"preconditioner", "diagonal"}, {"tolerance", "1e-10"}, {"relTol", "0"}, {"maxIter", "300"}});
        for (label step = 0; step <= steps; ++step) {
            if (step > 0) turbulence->correct(flowOf(step), rDeltaT, controls, kRelax);
            const std::string s = std::to_string(step);
            writeRaw(dir, "k_" + s, turbulence->k()); writeRaw(dir, "nuSgs_" + s, turbulence->nuSgs());
            writeRaw(dir, "bk_" + s, turbulence->kBoundary()); writeRaw(dir, "bnuSgs_" + s, turbulence->nuSgsBoundary());
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
