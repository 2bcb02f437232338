// scoped.h -- the one guard of the host files: a value written for the length of a scope.  Scoped<T> g(ref, v) keeps what `ref` held, writes v, and
// puts the kept value back when it goes, on every way out of the scope.  No device header: the host compiler alone builds it.
#pragma once
#include <utility>

namespace xfr {

template <class T>
class Scoped {
    T& ref;
    T prev;
public:
    template <class U>
    Scoped(T& r, U&& v) : ref(r), prev(std::move(r)) { ref = std::forward<U>(v); }
    ~Scoped() { ref = std::move(prev); }
    Scoped(const Scoped&) = delete;
    Scoped& operator=(const Scoped&) = delete;
};

}  // namespace xfr
