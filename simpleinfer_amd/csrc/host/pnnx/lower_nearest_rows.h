// pnnx/lower_nearest_rows.h -- the codebook lookup of a VQ encoder,
//     d = torch.cdist(z, codebook)        p = 2, codebook a pnnx.Attribute [Kc, M]
//     i = torch.argmin(d, dim=-1)         keepdim=False, the only reader of d
//     q = F.embedding(i, codebook)        or nn.Embedding whose @weight has the codebook's bytes; the only reader of i
// is ONE operator for the engine: torch.cdist (z, codebook) -> q with the added parameter nearest_rows=1, which layer/cdist.cpp runs as one
// launch of si_hip_nearest_* (include/si_nearest.h) that writes the winning rows alone.  The rewrite happens in the graph, before layers are
// created and before the batch rule looks at it: the engine has no integer tensors, so d and i never exist, and torch.argmin, F.embedding
// and nn.Embedding are no layer types.
#ifndef SIMPLEINFER_AMD_PNNX_LOWER_NEAREST_ROWS_H_
#define SIMPLEINFER_AMD_PNNX_LOWER_NEAREST_ROWS_H_

#include <string>

#include "ir.h"

namespace pnnx {

// returns the number of chains rewritten, or -1 with `why` (the operator and the condition it misses) when the graph holds a torch.argmin,
// F.embedding or nn.Embedding that is not part of such a chain: nothing else can run it.  Chains rewritten before the miss stay rewritten.
int lower_nearest_rows(Graph& graph, std::string* why = nullptr);

}  // namespace pnnx

#endif
