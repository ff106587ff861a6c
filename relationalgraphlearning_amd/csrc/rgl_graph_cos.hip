// rgl_graph_cos.hip -- the graph kernel's builds for the cosine family's passes (norm 4-5: cosine, cosine_softmax).
#include "rgl_graph_kernel.h"

namespace rgl {
namespace tiles {

int launch_graph_cos(const GraphArgs& ga, const GraphForm& f, int L, bool bwd, size_t lds, int grid, hipStream_t st) {
    return launch_graph_family<true, false>(ga, f, L, bwd, lds, grid, st);
}

}  // namespace tiles
}  // namespace rgl
