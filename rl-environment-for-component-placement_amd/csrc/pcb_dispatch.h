// pcb_dispatch.h -- the walk over a kernel family's candidate builds, stated once for the three families compiled per
// environment kind and part (pcb_launch.h: StepFamily, PlayoutFamily, GatherPathsFamily).  Included by the units that
// hold kernels (pcb_kind.inc, pcb_playout.inc, pcb_gather_paths.inc), each of which defines F::launch<KIND, I> for its
// family and ends with PCB_UNIT(F, part): the explicit instantiation of launch_in_unit for the kind and part it was compiled
// with (-DPCB_KIND=, [-DPCB_PART=n]; no PCB_PART = a kind without routes -- square, rect -- whose one unit is part 0).
#pragma once
#include <utility>

#include "pcb_launch.h"

#ifndef PCB_PART
#define PCB_PART 0
#endif

// Candidate I of family F: compiled here if this unit is its part, launched if it is b.
template <class F, int KIND, int PART, int I> static inline bool launch_if(const typename F::Launch &a, const typename F::Build &b) {
    if constexpr (F::part(KIND, F::build_at(I)) == PART) {
        if (pcb_layout::build_index(b) != I) return false;
        F::template launch<KIND, I>(a);
        return true;
    }
    return false;
}
template <class F, int KIND, int PART, int... I>
static inline bool launch_one_of(const typename F::Launch &a, const typename F::Build &b, std::integer_sequence<int, I...>) {
    return (launch_if<F, KIND, PART, I>(a, b) || ...);
}
template <class F, int KIND, int PART> int launch_in_unit(const typename F::Launch &a, const typename F::Build &b) {
    return launch_one_of<F, KIND, PART>(a, b, std::make_integer_sequence<int, F::builds>{}) ? 0 : -1;
}
#define PCB_UNIT(F, part) template int launch_in_unit<F, PCB_KIND, part>(const F::Launch &, const F::Build &);
