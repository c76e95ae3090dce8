// The DPP-row instantiations (template parameter DR of pcg_resident_kernel) of the plain and the cluster launches: a translation
// unit of their own, so that they compile beside those of gato_pcg_resident.hip instead of after them.
#include "gato_pcg_resident_launch.h"

namespace gato {

// `a` arrives checked and normalised by launch_pcg_resident.
template <typename T, int S>
int launch_pcg_resident_dpp(const PcgLaunch &a, hipStream_t st)
{
    if constexpr (DppRows<S>::ok) return launch_plain<T, S, true>(a, a.xslots != nullptr, a.k_end - a.k_begin, st);
    else {
        set_error("pcg_resident: no DPP-row layout for STATE_SIZE %d", S);
        return GATO_EINVAL;
    }
}
#define X(S_, C_)                                                          \
    template int launch_pcg_resident_dpp<float, S_>(const PcgLaunch &, hipStream_t); \
    template int launch_pcg_resident_dpp<double, S_>(const PcgLaunch &, hipStream_t);
GATO_SHAPES(X)
#undef X

}  // namespace gato
