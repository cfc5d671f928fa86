// Table launches: up to N entries (the argument sets of N streams, sessions, windows ...) travel BY VALUE as one kernel
// argument, a grid axis selects the entry, and blocks past an entry's own extent return at once.  One entry is a table of one.
#pragma once
#include <algorithm>

namespace css {

// A kernel's table type is a named struct derived from this, so that the kernel's symbol names the table, not its layout:
//   struct WindowTable : Table<WindowItem, WINDOW_MULTI_MAX> {};
template <class E, int N_>
struct Table {
    static_assert(sizeof(E) * N_ <= 4096, "the table travels by value as a kernel argument");
    static constexpr int N = N_;
    E e[N_];
};

// Entries entry(0) .. entry(n - 1), T::N per table of type T: launch(table, count) computes the grid and the LDS of the count
// entries it is handed and launches; it returns false to stop (the launcher's own failure), which is then what this returns.
template <class T, class Entry, class Launch>
bool for_each_table(int n, Entry&& entry, Launch&& launch) {
    for (int i0 = 0; i0 < n; i0 += T::N) {
        const int cnt = std::min(T::N, n - i0);
        T tab{};
        for (int i = 0; i < cnt; ++i) tab.e[i] = entry(i0 + i);
        if (!launch(tab, cnt)) return false;
    }
    return true;
}
// the same over an array of entries
template <class T, class E, class Launch>
bool for_each_table(const E* e, int n, Launch&& launch) {
    return for_each_table<T>(n, [&](int i) -> const E& { return e[i]; }, launch);
}

// the largest extent(entry) of a table's first cnt entries, at least `least`
template <class T, class E, int N, class Extent>
T table_max(const Table<E, N>& tab, int cnt, T least, Extent&& extent) {
    for (int i = 0; i < cnt; ++i) least = std::max<T>(least, extent(tab.e[i]));
    return least;
}

}  // namespace css
