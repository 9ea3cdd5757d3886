// Runtime value -> template argument, and the one way a template kernel is launched.
#pragma once
#include <type_traits>

#include "mdb_common.h"

// f(std::integral_constant<int, V>) for the first V of the list that equals v. mdb_pick: a value outside the list takes the LAST V (the
// final `else` / `default:` of a ladder); mdb_pick_or: it takes miss() instead (a ladder that ends in an error)
template <int V, int... Vs, class F, class E>
inline mdb_status mdb_pick_or(int v, F&& f, E&& miss) {
    if (v == V) return f(std::integral_constant<int, V>{});
    if constexpr (sizeof...(Vs) > 0) return mdb_pick_or<Vs...>(v, f, miss);
    else return miss();
}
template <int V, int... Vs, class F>
inline mdb_status mdb_pick(int v, F&& f) {
    if constexpr (sizeof...(Vs) > 0) {
        if (v != V) return mdb_pick<Vs...>(v, f);
    }
    return f(std::integral_constant<int, V>{});
}
template <class F>
inline mdb_status mdb_pick_bool(bool v, F&& f) {
    return v ? f(std::true_type{}) : f(std::false_type{});
}

// raises the kernel's dynamic LDS limit when this launch needs more than the default 48 KB (on every such launch: the limit is not cached),
// then launches on the context's stream; the launch error is the caller's hipGetLastError to collect
template <class... P, class... A>
inline mdb_status mdb_launch(mdb_ctx* ctx, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, const A&... args) {
    if (lds > 48 * 1024) MDB_HIP(ctx, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kernel<<<grid, block, lds, ctx->stream>>>(args...);
    return MDB_OK;
}
