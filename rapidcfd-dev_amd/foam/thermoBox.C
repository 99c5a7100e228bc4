// thermoBox -- a test driver, not an application: it runs the mirror's hePsiThermo (its constructor and three calls of correct()) on a case
// that tests/test_thermo.py writes as one raw file, and writes T, psi, mu, alpha, rho and the boundary values of T, psi, mu, alpha and he
// back after the constructor (step 0) and after every correct().  Between two calls he and p, with their boundary values, are changed by a
// fixed rule in exactly rounded operations: before correct() number s, he *= 1 + 0.03125*s and p *= 1 - 0.015625*s.  The mixture is air, the
// numbers typed in below (no dictionary is read); the file chooses the energy form, the thermodynamics and the transport.
//   <in>   int32: n nf nPatches energy thermo transport, lower[nf], upper[nf], size[nPatches], kind[nPatches] (0 empty, 1 fixesValue,
//          2 other), the faceCells of every patch; float64: T[n], p[n], bT[nb], bp[nb]; native byte order
//   <out>  float64, per step: T psi mu alpha rho (n each), bT bpsi bmu balpha bhe (nb each)
#include "miFoam.H"

#include <cstdio>
#include <fstream>

using namespace Foam;

template <class T>
static std::vector<T> readRaw(std::ifstream& f, std::size_t count)
{
    std::vector<T> v(count);
    if (count && !f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T)))) FatalErrorIn("thermoBox", "the input file is too short");
    return v;
}
static void writeRaw(std::ofstream& f, const scalargpuField& x)
{
    const std::vector<scalar> h = x.asHost();
    f.write(reinterpret_cast<const char*>(h.data()), (std::streamsize)(h.size() * sizeof(scalar)));
}
static void scale(scalargpuField& x, scalar factor)
{
    std::vector<scalar> h = x.asHost();
    for (scalar& v : h) v = v * factor;
    x = h;
}

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: thermoBox <in> <out>\n"); return 2; }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        if (!in) FatalErrorIn("thermoBox", "cannot open the input file");
        const std::vector<label> head = readRaw<label>(in, 6);
        const label n = head[0], nf = head[1], nPatches = head[2];
        const labelList lower = readRaw<label>(in, (std::size_t)nf), upper = readRaw<label>(in, (std::size_t)nf);
        const std::vector<label> sizes = readRaw<label>(in, (std::size_t)nPatches), kinds = readRaw<label>(in, (std::size_t)nPatches);
        std::vector<labelList> faceCells;
        std::vector<hePsiThermo::patchType> types;
        label nb = 0;
        for (label p = 0; p < nPatches; ++p) {
            faceCells.push_back(readRaw<label>(in, (std::size_t)sizes[(std::size_t)p]));
            types.push_back((hePsiThermo::patchType)kinds[(std::size_t)p]);
            nb += sizes[(std::size_t)p];
        }
        const scalargpuField T0(readRaw<scalar>(in, (std::size_t)n));
        scalargpuField p(readRaw<scalar>(in, (std::size_t)n));
        const scalargpuField bT0(readRaw<scalar>(in, (std::size_t)nb));
        scalargpuField bp(readRaw<scalar>(in, (std::size_t)nb));
        // air: hConst {Cp, Hf} | eConst {Cv, Hf} | janaf {Tlow, Thigh, Tcommon, high, low}; const {mu, Pr} | sutherland {As, Ts}
        const double hConst[2] = {1007.0, 0.0}, eConst[2] = {719.3, 0.0};
        const double janaf[17] = {200.0, 6000.0, 1000.0, 3.08792717, 0.00124597184, -4.23718945e-07, 6.74774789e-11, -3.97076972e-15, -995.262755, 5.9596093,
                                  3.5683962, -0.000678729429, 1.55371476e-06, -3.2993706e-12, -4.66395387e-13, -1062.34659, 3.71582965};
        const double constTransport[2] = {1.84e-05, 0.7}, sutherland[2] = {1.4792e-06, 116.0};
        mi_thermo_model model;
        if (mi_thermo_model_init(head[3], head[4], head[5], 28.9, head[4] == MI_THERMO_HCONST ? hConst : head[4] == MI_THERMO_ECONST ? eConst : janaf,
                                 head[5] == MI_THERMO_CONST ? constTransport : sutherland, &model) != 0)
            FatalErrorIn("thermoBox", std::string("mi_thermo_model_init: ") + mi_last_error());
        const std::vector<gradBoundary::patchKind> gradKinds((std::size_t)nPatches, gradBoundary::other);
        lduAddressing addr(n, lower, upper);
        gradBoundary boundary(addr, faceCells, gradKinds);
        std::ofstream out(argv[2], std::ios::binary);
        hePsiThermo thermo(addr, boundary, sizes, types, model, p, bp, T0, bT0);
        for (int step = 0; step <= 3; ++step) {
            if (step) {
                scale(thermo.he(), 1.0 + 0.03125 * step); scale(thermo.heBoundary(), 1.0 + 0.03125 * step);
                scale(p, 1.0 - 0.015625 * step); scale(bp, 1.0 - 0.015625 * step);
                thermo.correct();
            }
            writeRaw(out, thermo.T()); writeRaw(out, thermo.psi()); writeRaw(out, thermo.mu()); writeRaw(out, thermo.alpha()); writeRaw(out, thermo.rho());
            writeRaw(out, thermo.TBoundary()); writeRaw(out, thermo.psiBoundary()); writeRaw(out, thermo.muBoundary()); writeRaw(out, thermo.alphaBoundary());
            writeRaw(out, thermo.heBoundary());
        }
        if (!out) FatalErrorIn("thermoBox", "cannot write the output file");
        std::printf("thermoBox ok: %d cells, %d boundary faces\n", (int)n, (int)nb);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "thermoBox: %s\n", e.what());
        return 1;
    }
}
