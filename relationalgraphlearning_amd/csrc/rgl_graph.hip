// rgl_graph.hip -- which build of the graph kernel (rgl_graph_kernel.h) a graph launch takes, on how many workgroups, and the launch
// itself: the kernels are compiled a family to a translation unit (rgl_graph_plain.hip, rgl_graph_cos.hip, rgl_graph_lw.hip).
#include "rgl_graph_kernel.h"

namespace rgl {
namespace tiles {

// the instantiation a graph launch takes -- decided HERE, read by plan_graph, launch_graph and rgl_plan_graph_tiles:
// node tiles by N, feature tiles by x_dim (32 | 64), the family by the normalisation and the layerwise flag of graph_args
GraphForm graph_form(int N, int X, int norm, bool lw) {
    return GraphForm{N <= 16 ? 1 : (N <= 32 ? 2 : 4), X == 32 ? 2 : 4, lw ? 2 : (norm >= 4 ? 1 : 0)};
}

template <int NT, int XT>
GraphPlan plan_graph_nx(int S, int N, int L, bool bwd, bool lw) {
    GraphPlan p{};
    p.lds = (size_t)(GraphLds<NT, XT>::weight_floats(L) + GraphLds<NT, XT>::scene_floats(N, L, bwd, lw)) * sizeof(float);
    if (p.lds > (size_t)rgl::kLdsBytesPerCu) return p;
    // persistent workgroups: as many as are resident at once (LDS, and the waves the kernel's register budget allows), scenes dealt
    // round robin
    const int by_waves = lw ? 2 : ((NT == 2 && XT == 2) ? 16 : (NT == 1 ? 12 : 8)) / (2 * NT);
    int per_cu = workgroups_per_cu_by_lds(p.lds, by_waves);
    per_cu = per_cu < 1 ? 1 : per_cu;
    p.resident = kCuCount * per_cu;
    p.grid = S < p.resident ? S : p.resident;
    return p;
}
// x_dim 32 or 64
GraphPlan plan_graph(int S, int N, int X, int L, bool bwd, bool lw) {
    const GraphForm f = graph_form(N, X, 0, lw);
    switch (f.nt * 10 + f.xt) {
        case 12: return plan_graph_nx<1, 2>(S, N, L, bwd, lw);
        case 22: return plan_graph_nx<2, 2>(S, N, L, bwd, lw);
        case 42: return plan_graph_nx<4, 2>(S, N, L, bwd, lw);
        case 14: return plan_graph_nx<1, 4>(S, N, L, bwd, lw);
        case 24: return plan_graph_nx<2, 4>(S, N, L, bwd, lw);
        default: return plan_graph_nx<4, 4>(S, N, L, bwd, lw);
    }
}
// the backward's launch while the caller's workspace is short: a slab per workgroup, at most `max_workgroups` of them
GraphPlan cap_graph_plan(GraphPlan p, int max_workgroups) {
    p.grid = p.grid < max_workgroups ? p.grid : max_workgroups;
    return p;
}
int launch_graph(const GraphArgs& ga, int X, int L, bool bwd, const GraphPlan& p, hipStream_t st) {
    const GraphForm f = graph_form(ga.N, X, ga.norm, ga.lw != 0);
    switch (f.family) {
        case 2: return launch_graph_lw(ga, f, L, bwd, p.lds, p.grid, st);
        case 1: return launch_graph_cos(ga, f, L, bwd, p.lds, p.grid, st);
        default: return launch_graph_plain(ga, f, L, bwd, p.lds, p.grid, st);
    }
}

}  // namespace tiles
}  // namespace rgl
