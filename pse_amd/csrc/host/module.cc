// pybind11 module _PSEv1: the classes the reference registers at PSEv1/module.cc:13-22 (export_Stokes,
// export_ShearFunction, export_ShearFunctionWrap, export_SpecificShearFunction, export_VariantShearFunction), with the
// same Python names.  Device arrays are passed as integer addresses (torch tensor .data_ptr()).
#include <pybind11/pybind11.h>

#include "ShearFunction.h"
#include "Stokes.h"

namespace py = pybind11;
using namespace pse_host;

// trampoline so Python subclasses can override (the reference's ShearFunctionWrap binds the base class methods and has
// no trampoline, so overriding silently does nothing there -- SURVEY.md 2.4-10)
class ShearFunctionWrap : public ShearFunction {
public:
    using ShearFunction::ShearFunction;
    double getShearRate(unsigned int t) override { PYBIND11_OVERRIDE(double, ShearFunction, getShearRate, t); }
    double getStrain(unsigned int t) override { PYBIND11_OVERRIDE(double, ShearFunction, getStrain, t); }
    unsigned int getOffset() override { PYBIND11_OVERRIDE(unsigned int, ShearFunction, getOffset, ); }
};

template <class T>
static T *ptr(std::uintptr_t a) { return reinterpret_cast<T *>(a); }

PYBIND11_MODULE(_PSEv1, m) {
    py::class_<ShearFunction, ShearFunctionWrap, std::shared_ptr<ShearFunction>>(m, "ShearFunction")
        .def(py::init<>())
        .def("getShearRate", &ShearFunction::getShearRate)
        .def("getStrain", &ShearFunction::getStrain)
        .def("getOffset", &ShearFunction::getOffset);
    m.attr("ShearFunctionWrap") = m.attr("ShearFunction");
    py::class_<SinShearFunction, ShearFunction, std::shared_ptr<SinShearFunction>>(m, "SinShearFunction")
        .def(py::init<double, double, unsigned int, double>());
    py::class_<SteadyShearFunction, ShearFunction, std::shared_ptr<SteadyShearFunction>>(m, "SteadyShearFunction")
        .def(py::init<double, unsigned int, double>());
    py::class_<ChirpShearFunction, ShearFunction, std::shared_ptr<ChirpShearFunction>>(m, "ChirpShearFunction")
        .def(py::init<double, double, double, double, unsigned int, double>());
    py::class_<TukeyWindowFunction, ShearFunction, std::shared_ptr<TukeyWindowFunction>>(m, "TukeyWindowFunction")
        .def(py::init<double, double, unsigned int, double>());
    py::class_<WindowedFunction, ShearFunction, std::shared_ptr<WindowedFunction>>(m, "WindowedFunction")
        .def(py::init<std::shared_ptr<ShearFunction>, std::shared_ptr<ShearFunction>>());

    py::class_<Variant, std::shared_ptr<Variant>>(m, "Variant").def("getValue", &Variant::getValue);
    py::class_<VariantConst, Variant, std::shared_ptr<VariantConst>>(m, "VariantConst").def(py::init<double>());
    py::class_<VariantShearFunction, Variant, std::shared_ptr<VariantShearFunction>>(m, "VariantShearFunction")
        .def(py::init<std::shared_ptr<ShearFunction>, unsigned int, double, double>())
        .def("wrapValue", &VariantShearFunction::wrapValue);

    py::class_<Stokes, std::shared_ptr<Stokes>>(m, "Stokes")
        .def(py::init([](unsigned int n_total, double Lx, double Ly, double Lz, double xy, std::shared_ptr<Variant> T,
                         unsigned int seed, double xi, double error, double dt) {
            return std::make_shared<Stokes>(n_total, BoxDim{Lx, Ly, Lz, xy}, T, seed, xi, error, dt);
        }))
        .def("setT", &Stokes::setT)
        .def("setParams", &Stokes::setParams)
        .def("setShear", &Stokes::setShear)
        .def("setDeltaT", &Stokes::setDeltaT)
        .def("setOverrides", &Stokes::setOverrides)
        .def("setLanczosOperator", &Stokes::setLanczosOperator)
        .def("setBox", [](Stokes &s, double Lx, double Ly, double Lz, double xy) { s.setBox(BoxDim{Lx, Ly, Lz, xy}); })
        .def("integrateStepOne", [](Stokes &s, unsigned int timestep, std::uintptr_t pos, std::uintptr_t vel, std::uintptr_t accel,
                                    std::uintptr_t image, std::uintptr_t force, std::uintptr_t group, unsigned int n) {
            s.integrateStepOne(timestep, ParticleArrays{ptr<pse_double4>(pos), ptr<pse_double4>(vel), ptr<pse_double3>(accel),
                                                       ptr<pse_int3>(image), ptr<const pse_double4>(force),
                                                       ptr<const unsigned int>(group), n});
        })
        .def("integrateStepTwo", &Stokes::integrateStepTwo)
        .def("pairRepulsion", [](Stokes &s, std::uintptr_t pos, std::uintptr_t force, std::uintptr_t group, unsigned int n, double k,
                                 double sigma, bool accumulate) {
            s.pairRepulsion(ptr<const pse_double4>(pos), ptr<pse_double4>(force), ptr<const unsigned int>(group), n, k, sigma, accumulate);
        })
        .def("pairRepulsionVirial", [](Stokes &s, std::uintptr_t pos, std::uintptr_t force, std::uintptr_t group, unsigned int n, double k,
                                       double sigma, bool accumulate, std::uintptr_t out8) {
            s.pairRepulsionVirial(ptr<const pse_double4>(pos), ptr<pse_double4>(force), ptr<const unsigned int>(group), n, k, sigma, accumulate,
                                  ptr<double>(out8));
        })
        .def("pairTable", [](Stokes &s, std::uintptr_t pos, std::uintptr_t force, std::uintptr_t group, unsigned int n, std::uintptr_t table,
                             int width, double rmin, double rmax, bool accumulate, std::uintptr_t out8) {
            s.pairTable(ptr<const pse_double4>(pos), ptr<pse_double4>(force), ptr<const unsigned int>(group), n, ptr<const double>(table), width,
                        rmin, rmax, accumulate, ptr<double>(out8));
        })
        // pair exclusions: npairs x 2 uint32 HOST indices by address (numpy .ctypes.data); the _excl passes take the id
        .def("exclusionsCreate", [](Stokes &s, unsigned int n, unsigned int npairs, std::uintptr_t pairs) {
            return s.exclusionsCreate(n, npairs, ptr<const unsigned int>(pairs));
        })
        .def("exclusionsDestroy", &Stokes::exclusionsDestroy)
        .def("pairTableExcl", [](Stokes &s, std::uintptr_t pos, std::uintptr_t force, std::uintptr_t group, unsigned int n, std::uintptr_t table,
                                 int width, double rmin, double rmax, bool accumulate, std::uintptr_t out8, int ex) {
            s.pairTableExcl(ptr<const pse_double4>(pos), ptr<pse_double4>(force), ptr<const unsigned int>(group), n, ptr<const double>(table),
                            width, rmin, rmax, accumulate, ptr<double>(out8), ex);
        })
        .def("pairRepulsionExcl", [](Stokes &s, std::uintptr_t pos, std::uintptr_t force, std::uintptr_t group, unsigned int n, double k,
                                     double sigma, bool accumulate, std::uintptr_t out8, int ex) {
            s.pairRepulsionExcl(ptr<const pse_double4>(pos), ptr<pse_double4>(force), ptr<const unsigned int>(group), n, k, sigma, accumulate,
                                ptr<double>(out8), ex);
        })
        // typed pair tables: HOST arrays by address (numpy .ctypes.data): n uint32 types, npt int32 widths, npt float64 rmin and rmax,
        // sum(width) x 2 float64 table entries; pairTableTyped takes the id, and the id of an exclusion object or -1
        .def("typedTableCreate", [](Stokes &s, unsigned int n, std::uintptr_t types, int ntypes, std::uintptr_t width, std::uintptr_t rmin,
                                    std::uintptr_t rmax, std::uintptr_t tables) {
            return s.typedTableCreate(n, ptr<const unsigned int>(types), ntypes, ptr<const int>(width), ptr<const double>(rmin),
                                      ptr<const double>(rmax), ptr<const double>(tables));
        })
        .def("typedTableDestroy", &Stokes::typedTableDestroy)
        .def("pairTableTyped", [](Stokes &s, std::uintptr_t pos, std::uintptr_t force, std::uintptr_t group, unsigned int n, bool accumulate,
                                  std::uintptr_t out8, int typed, int ex) {
            s.pairTableTyped(ptr<const pse_double4>(pos), ptr<pse_double4>(force), ptr<const unsigned int>(group), n, accumulate,
                             ptr<double>(out8), typed, ex);
        })
        // host arrays by address too (numpy .ctypes.data): nbonds x 2 uint32, nbonds uint32 or 0, ntypes int32 / float64 / float64
        .def("bondsCreate", [](Stokes &s, unsigned int n, unsigned int nbonds, std::uintptr_t pairs, std::uintptr_t types, int ntypes,
                               std::uintptr_t kind, std::uintptr_t k, std::uintptr_t r0) {
            return s.bondsCreate(n, nbonds, ptr<const unsigned int>(pairs), ptr<const unsigned int>(types), ntypes, ptr<const int>(kind),
                                 ptr<const double>(k), ptr<const double>(r0));
        })
        .def("bondForces", [](Stokes &s, int id, std::uintptr_t pos, std::uintptr_t force, bool accumulate, std::uintptr_t out8) {
            s.bondForces(id, ptr<const pse_double4>(pos), ptr<pse_double4>(force), accumulate, ptr<double>(out8));
        })
        .def("bondsOverstretched", &Stokes::bondsOverstretched)
        .def("bondsDestroy", &Stokes::bondsDestroy)
        // nangles x 3 uint32 (end, vertex, end), nangles uint32 or 0, ntypes int32 / float64 / float64
        .def("anglesCreate", [](Stokes &s, unsigned int n, unsigned int nangles, std::uintptr_t triples, std::uintptr_t types, int ntypes,
                                std::uintptr_t kind, std::uintptr_t k, std::uintptr_t theta0) {
            return s.anglesCreate(n, nangles, ptr<const unsigned int>(triples), ptr<const unsigned int>(types), ntypes, ptr<const int>(kind),
                                  ptr<const double>(k), ptr<const double>(theta0));
        })
        .def("angleForces", [](Stokes &s, int id, std::uintptr_t pos, std::uintptr_t force, bool accumulate, std::uintptr_t out8) {
            s.angleForces(id, ptr<const pse_double4>(pos), ptr<pse_double4>(force), accumulate, ptr<double>(out8));
        })
        .def("anglesDestroy", &Stokes::anglesDestroy)
        // ndihedrals x 4 uint32 (i, j, k, l), ndihedrals uint32 or 0, ntypes int32, ntypes x 4 float64
        .def("dihedralsCreate", [](Stokes &s, unsigned int n, unsigned int ndihedrals, std::uintptr_t quads, std::uintptr_t types, int ntypes,
                                   std::uintptr_t kind, std::uintptr_t params) {
            return s.dihedralsCreate(n, ndihedrals, ptr<const unsigned int>(quads), ptr<const unsigned int>(types), ntypes, ptr<const int>(kind),
                                     ptr<const double>(params));
        })
        .def("dihedralForces", [](Stokes &s, int id, std::uintptr_t pos, std::uintptr_t force, bool accumulate, std::uintptr_t out8) {
            s.dihedralForces(id, ptr<const pse_double4>(pos), ptr<pse_double4>(force), accumulate, ptr<double>(out8));
        })
        .def("dihedralsDestroy", &Stokes::dihedralsDestroy)
        .def("lanczosIterations", &Stokes::lanczosIterations)
        .def("hashedSeed", &Stokes::hashedSeed)
        .def("info", [](const Stokes &s) {
            const pse_info i = s.info();
            py::dict d;
            d["Nx"] = i.Nx; d["Ny"] = i.Ny; d["Nz"] = i.Nz; d["P"] = i.P; d["rcut"] = i.rcut; d["xi"] = i.xi; d["eta"] = i.eta;
            d["gaussm"] = i.gaussm; d["self_mobility"] = i.self_mobility; d["lanczos_m"] = i.lanczos_m;
            return d;
        });
}
