// rgl_graph_lw.hip -- the graph kernel's builds for layerwise graphs (an adjacency per layer; x_dim 32, N <= 32).
#include "rgl_graph_kernel.h"

namespace rgl {
namespace tiles {

int launch_graph_lw(const GraphArgs& ga, const GraphForm& f, int L, bool bwd, size_t lds, int grid, hipStream_t st) {
    return launch_graph_family<false, true>(ga, f, L, bwd, lds, grid, st);
}

}  // namespace tiles
}  // namespace rgl
