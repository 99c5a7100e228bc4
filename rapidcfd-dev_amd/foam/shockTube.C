// shockTube -- a test driver, not an application: the inviscid statements of rhoCentralFoam.C on a one-dimensional tube of <n> cells of unit
// cross-section along x in [-5, 5], with the standard shock-tube states (left p = 1e5, T = 348.4; right p = 1e4, T = 278.2; U = 0), air as
// eConst / perfectGas (the numbers typed in below, no dictionary is read), Kurganov with vanLeer / vanLeerV / vanLeer, deltaT = 1e-5 fixed.
// Every step runs rhoCentralFoam.C:60-257 without the viscous branch: the fluxes (centralFluxes::update), the Courant number, the three explicit
// solve(fvm::ddt + fvc::div) (centralFluxes::solveDdtDiv), U, e, thermo.correct() through the mirror's hePsiThermo and p.  The two end patches
// are zeroGradient; the empty side patches of a one-dimensional case are left out.  Host glue, where the engine has no entry: the boundary
// fields of the two end faces (the cell's value; rhoU_b = rho_b*U_b, rho_b = psi_b*p_b as the reference assigns them) and
// e = rhoE/rho - 0.5*magSqr(U) after the division (every operator rounded; U_y = U_z = 0 here, so the contraction of magSqr changes no bit).
// rhoE's boundary field is read by nothing in the inviscid branch and is not kept.
//   <out>  float64, per step: phi phiEp amaxSf (n - 1 each), the boundary phi (2), rho rhoU_x rhoE e T psi p (n each), CoNum, meanCoNum
#include "miFoam.H"

#include <cstdio>
#include <cstdlib>
#include <fstream>

using namespace Foam;

static void writeRaw(std::ofstream& f, const scalargpuField& x)
{
    const std::vector<scalar> h = x.asHost();
    f.write(reinterpret_cast<const char*>(h.data()), (std::streamsize)(h.size() * sizeof(scalar)));
}
// the values of a cell field at the two end cells: a zeroGradient patch field
static std::vector<scalar> ends(const scalargpuField& x)
{
    const std::vector<scalar> h = x.asHost();
    return {h.front(), h.back()};
}
static void setVector(vectorgpuField& v, const std::vector<scalar>& x, const std::vector<scalar>& y, const std::vector<scalar>& z)
{
    v.c[0] = x; v.c[1] = y; v.c[2] = z;
}

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: shockTube <cells> <steps> <out>\n"); return 2; }
    try {
        const label n = std::atoi(argv[1]), steps = std::atoi(argv[2]);
        if (n < 2 || steps < 1) FatalErrorIn("shockTube", "at least two cells and one step");
        const label nf = n - 1;
        const scalar length = 10.0, h = length / n, deltaT = 1.0e-5, rDeltaT = 1.0 / deltaT;
        labelList lower((std::size_t)nf), upper((std::size_t)nf);
        for (label f = 0; f < nf; ++f) { lower[(std::size_t)f] = f; upper[(std::size_t)f] = f + 1; }
        const std::vector<labelList> faceCells = {{0}, {n - 1}};
        const std::vector<scalar> one((std::size_t)nf, 1.0), zero((std::size_t)nf, 0.0), zeroC((std::size_t)n, 0.0), zeroB(2, 0.0);
        std::vector<scalar> x((std::size_t)n), p0((std::size_t)n), T0((std::size_t)n);
        for (label i = 0; i < n; ++i) {
            x[(std::size_t)i] = (i + 0.5) * h - 0.5 * length;
            const bool left = x[(std::size_t)i] < 0;
            p0[(std::size_t)i] = left ? 1.0e5 : 1.0e4;
            T0[(std::size_t)i] = left ? 348.4 : 278.2;
        }
        const scalargpuField weights(std::vector<scalar>((std::size_t)nf, 0.5)), magSf(one), deltaCoeffs(std::vector<scalar>((std::size_t)nf, 1.0 / h));
        const scalargpuField V(std::vector<scalar>((std::size_t)n, h)), bMagSf(std::vector<scalar>(2, 1.0)), bDeltaCoeffs(std::vector<scalar>(2, 2.0 / h));
        vectorgpuField Sf(nf), C(n), bSf(2);
        setVector(Sf, one, zero, zero); setVector(C, x, zeroC, zeroC); setVector(bSf, {-1.0, 1.0}, zeroB, zeroB);
        const scalar sumMagSf = (scalar)nf;

        const double eConst[2] = {717.5, 0.0}, constTransport[2] = {1.8e-05, 0.7};
        mi_thermo_model model;
        if (mi_thermo_model_init(MI_THERMO_INTERNAL_ENERGY, MI_THERMO_ECONST, MI_THERMO_CONST, 28.96, eConst, constTransport, &model) != 0)
            FatalErrorIn("shockTube", std::string("mi_thermo_model_init: ") + mi_last_error());
        lduAddressing addr(n, lower, upper);
        gradBoundary boundary(addr, faceCells, {gradBoundary::other, gradBoundary::other});
        scalargpuField p(p0), bp(std::vector<scalar>{p0.front(), p0.back()});
        hePsiThermo thermo(addr, boundary, {1, 1}, {hePsiThermo::other, hePsiThermo::other}, model, p, bp, scalargpuField(T0),
                           scalargpuField(std::vector<scalar>{T0.front(), T0.back()}));
        centralFluxes fluxes(addr, faceCells, "Kurganov", "vanLeer", "vanLeerV", "vanLeer",
                             centralFluxes::geometry{weights, Sf, magSf, deltaCoeffs, C, V, bSf, bMagSf, bDeltaCoeffs});

        // createFields.H: rho = thermo.rho() = psi*p, rhoU = rho*U, rhoE = rho*(e + 0.5*magSqr(U)) with U = 0
        std::vector<scalar> hr = thermo.psi().asHost(), hE((std::size_t)n);
        {
            const std::vector<scalar> he = thermo.he().asHost();
            for (label i = 0; i < n; ++i) { hr[(std::size_t)i] = hr[(std::size_t)i] * p0[(std::size_t)i]; hE[(std::size_t)i] = hr[(std::size_t)i] * (he[(std::size_t)i] + 0.5 * 0.0); }
        }
        scalargpuField rho(hr), rhoE(hE), q(n), Cp(n), Cv(n), bCp(2), bCv(2);
        vectorgpuField rhoU(n), U(n), brhoU(2);
        std::vector<scalar> bpsi = thermo.psiBoundary().asHost(), hbp = bp.asHost();
        scalargpuField brho(std::vector<scalar>{bpsi[0] * hbp[0], bpsi[1] * hbp[1]});

        std::ofstream out(argv[3], std::ios::binary);
        for (label step = 0; step < steps; ++step) {
            thermo.Cp(Cp, bCp); thermo.Cv(Cv, bCv);
            fluxes.update(centralFluxes::volFields{rho, rhoU, thermo.psi(), thermo.he(), Cp, Cv},
                          centralFluxes::volFields{brho, brhoU, thermo.psiBoundary(), thermo.heBoundary(), bCp, bCv});
            scalar CoNum = 0.0, meanCoNum = 0.0;
            fluxes.CourantNo(deltaT, sumMagSf, CoNum, meanCoNum);
            writeRaw(out, fluxes.phi()); writeRaw(out, fluxes.phiEp()); writeRaw(out, fluxes.amaxSf()); writeRaw(out, fluxes.phiBoundary());
            fluxes.solveDdtDiv(rho, rDeltaT, fluxes.phi(), fluxes.phiBoundary());                                  // :191
            for (direction d = 0; d < 3; ++d) fluxes.solveDdtDiv(rhoU.c[d], rDeltaT, fluxes.phiUp().c[d], fluxes.phiUpBoundary().c[d]);   // :194
            for (direction d = 0; d < 3; ++d) fieldDivide(U.c[d], rhoU.c[d], rho);                                 // :196-198
            const std::vector<scalar> rb = ends(rho);                                                              // zeroGradient after the solve
            for (direction d = 0; d < 3; ++d) { const std::vector<scalar> ub = ends(U.c[d]); brhoU.c[d] = std::vector<scalar>{rb[0] * ub[0], rb[1] * ub[1]}; }   // :199-200
            fluxes.solveDdtDiv(rhoE, rDeltaT, fluxes.phiEp(), fluxes.phiEpBoundary());                             // :226-231 without sigmaDotU
            fieldDivide(q, rhoE, rho);                                                                             // :233
            {
                std::vector<scalar> e = q.asHost();
                const std::vector<scalar> ux = U.c[0].asHost(), uy = U.c[1].asHost(), uz = U.c[2].asHost();
                for (label i = 0; i < n; ++i) {
                    const std::size_t k = (std::size_t)i;
                    const scalar a = ux[k] * ux[k], b = uy[k] * uy[k], c = uz[k] * uz[k], m = (a + b) + c, half = 0.5 * m;
                    e[k] = e[k] - half;
                }
                thermo.he() = e;
                thermo.heBoundary() = std::vector<scalar>{e.front(), e.back()};                                   // :234
            }
            thermo.correct();                                                                                      // :235
            fieldDivide(p, rho, thermo.psi());                                                                     // :253-255
            const std::vector<scalar> pb = ends(p);
            bp = pb;                                                                                               // :256
            bpsi = thermo.psiBoundary().asHost();
            brho = std::vector<scalar>{bpsi[0] * pb[0], bpsi[1] * pb[1]};                                          // :257
            writeRaw(out, rho); writeRaw(out, rhoU.c[0]); writeRaw(out, rhoE); writeRaw(out, thermo.he()); writeRaw(out, thermo.T());
            writeRaw(out, thermo.psi()); writeRaw(out, p);
            out.write(reinterpret_cast<const char*>(&CoNum), sizeof(scalar)); out.write(reinterpret_cast<const char*>(&meanCoNum), sizeof(scalar));
        }
        if (!out) FatalErrorIn("shockTube", "cannot write the output file");
        std::printf("shockTube ok: %d cells, %d steps\n", (int)n, (int)steps);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "shockTube: %s\n", e.what());
        return 1;
    }
}
