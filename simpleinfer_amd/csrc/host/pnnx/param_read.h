// pnnx/param_read.h -- typed readers for an operator's parameters, used by the layers' Init.  Depends on ir.h alone.
//
// Every reader returns false and leaves its output untouched when the key is missing or holds another type.
#ifndef SIMPLEINFER_AMD_PNNX_PARAM_READ_H_
#define SIMPLEINFER_AMD_PNNX_PARAM_READ_H_

#include <string>
#include <vector>

#include "ir.h"

namespace SimpleInfer {

// the parameter under `key`; nullptr when there is none.  `type` >= 0: and when it holds another type (ir.h: 1=b 2=i 3=f 4=s 5=ai)
static inline const pnnx::Parameter* FindParam(const pnnx::Operator* op, const char* key, int type = -1) {
    if (!op) return nullptr;
    auto it = op->params.find(key);
    return it != op->params.end() && (type < 0 || it->second.type == type) ? &it->second : nullptr;
}

// ---- required values ------------------------------------------------------------------------------------------------------
static inline bool Get(const pnnx::Operator* op, const char* key, bool& v) {
    const pnnx::Parameter* p = FindParam(op, key, 1);
    if (p) v = p->b;
    return p != nullptr;
}
static inline bool Get(const pnnx::Operator* op, const char* key, int& v) {
    const pnnx::Parameter* p = FindParam(op, key, 2);
    if (p) v = p->i;
    return p != nullptr;
}
static inline bool Get(const pnnx::Operator* op, const char* key, float& v) {
    const pnnx::Parameter* p = FindParam(op, key, 3);
    if (p) v = p->f;
    return p != nullptr;
}
static inline bool Get(const pnnx::Operator* op, const char* key, std::string& v) {
    const pnnx::Parameter* p = FindParam(op, key, 4);
    if (p) v = p->s;
    return p != nullptr;
}
static inline bool Get(const pnnx::Operator* op, const char* key, std::vector<int>& v) {
    const pnnx::Parameter* p = FindParam(op, key, 5);
    if (p) v = p->ai;
    return p != nullptr;
}

// ---- optional values ------------------------------------------------------------------------------------------------------
// Two rules for "not given" live in the layers, and model files load by them, so both stay:
//   IsNone        a missing key or type 0.  The string "None" is a value here (Pad2d, Upsample: the typed read that follows refuses it).
//   IsNoneOrText  the same, or the string "None" (ParamActivation, Slice: Number / OptionalInt below).
static inline bool IsNone(const pnnx::Operator* op, const char* key) {
    const pnnx::Parameter* p = FindParam(op, key);
    return !p || 0 == p->type;
}
static inline bool IsNoneOrText(const pnnx::Operator* op, const char* key) {
    const pnnx::Parameter* p = FindParam(op, key, 4);
    return IsNone(op, key) || (p && p->s == "None");
}

// a float the file may write as a float or an int
static inline bool GetNumber(const pnnx::Operator* op, const char* key, float& v) {
    int i = 0;
    if (Get(op, key, v)) return true;
    if (!Get(op, key, i)) return false;
    v = (float)i;
    return true;
}

// the optional forms: not given (IsNoneOrText) is fine and leaves `have` false; another type is an error
static inline bool Number(const pnnx::Operator* op, const char* key, float& v, bool& have) {
    have = !IsNoneOrText(op, key) && GetNumber(op, key, v);
    return have || IsNoneOrText(op, key);
}
static inline bool OptionalInt(const pnnx::Operator* op, const char* key, int& v, bool& have) {
    have = !IsNoneOrText(op, key) && Get(op, key, v);
    return have || IsNoneOrText(op, key);
}

}  // namespace SimpleInfer

#endif
