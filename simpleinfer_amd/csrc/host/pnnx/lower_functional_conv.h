// pnnx/lower_functional_conv.h -- F.conv2d whose filter (and bias, if any) are graph constants with no other reader is the module nn.Conv2d
// written as a function: the operator is rewritten to nn.Conv2d in the graph, before layers are created and before the batch rule sees it, so
// that every Conv2d route, fusion, fp16 rule and group count applies and the bits are those of the same nn.Conv2d by construction.
#ifndef SIMPLEINFER_AMD_PNNX_LOWER_FUNCTIONAL_CONV_H_
#define SIMPLEINFER_AMD_PNNX_LOWER_FUNCTIONAL_CONV_H_

#include "ir.h"

namespace pnnx {

// returns the number of operators rewritten.  Touches F.conv2d operators alone (and the pnnx.Attribute operators they were the only reader
// of, which leave the graph); an operator it cannot express as nn.Conv2d (a constant with another reader, an asymmetric 'same' pad, shapes
// that disagree) stays as it is.
int lower_functional_conv(Graph& graph);

}  // namespace pnnx

#endif
