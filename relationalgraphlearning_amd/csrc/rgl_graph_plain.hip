// rgl_graph_plain.hip -- the graph kernel's builds for the softmax, squared, equal_attention and diagonal normalisations (norm 0-3), one adjacency for all layers.
#include "rgl_graph_kernel.h"

namespace rgl {
namespace tiles {

int launch_graph_plain(const GraphArgs& ga, const GraphForm& f, int L, bool bwd, size_t lds, int grid, hipStream_t st) {
    return launch_graph_family<false, false>(ga, f, L, bwd, lds, grid, st);
}

}  // namespace tiles
}  // namespace rgl
