// engine_internal.h -- shared by the translation units of EngineImpl (engine_impl.cpp, engine_plan.cpp, engine_split.cpp) and by nothing else.
#ifndef SIMPLE_INFER_SRC_ENGINE_INTERNAL_H_
#define SIMPLE_INFER_SRC_ENGINE_INTERNAL_H_

#include "logger.h"
#include "si_hip.h"
#include "types.h"

#define SI_TRY_HIP(expr, what)                                             \
    {                                                                      \
        const int _rc = (expr);                                            \
        if (_rc != 0) {                                                    \
            LOG(ERROR) << what << ": " << si_hip_error_string(_rc);        \
            return Status::kFail;                                          \
        }                                                                  \
    }

#endif
