// Drives desire_amd/csrc/workspace.h over a counting fake allocator (tests/test_workspace.py).  One request per line on stdin; every answer ends
// with the allocator's counters and the number of entries:  ... <allocs> <frees> <entries>
//   in:  fail_at n                        the n-th allocation from now fails (0: none)     out: ok <a> <f> <e>
//   in:  ensure name bytes                out: <rc> <fresh> <a> <f> <e>
//   in:  ensure_all k name bytes ..       out: <rc> <failed name, or -> <a> <f> <e>
//   in:  get name                         out: <get() as an integer> <bytes()> <find() != nullptr> <find()->p == get()> <a> <f> <e>
//   in:  release_all                      out: ok <a> <f> <e>
// An exception ends the driver with a non-zero status (nothing in workspace.h may throw on a lookup).
#include "workspace.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static long g_allocs = 0, g_frees = 0, g_fail_in = 0;
static int fake_alloc(void** p, size_t bytes) {
    if (g_fail_in > 0 && --g_fail_in == 0) { *p = nullptr; return -1; }
    *p = std::malloc(bytes);
    ++g_allocs;
    return *p ? 0 : -1;
}
static void fake_free(void* p) { std::free(p); ++g_frees; }

int main() {
    Workspace ws(fake_alloc, fake_free);
    const Workspace& cws = ws;                               // lookups go through the const interface: they cannot insert
    auto tail = [&]() { std::printf(" %ld %ld %zu\n", g_allocs, g_frees, cws.size()); };
    char cmd[16], name[64];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "fail_at")) {
            if (std::scanf("%ld", &g_fail_in) != 1) return 1;
            std::printf("ok");
        } else if (!std::strcmp(cmd, "ensure")) {
            size_t bytes;
            if (std::scanf("%63s %zu", name, &bytes) != 2) return 1;
            bool fresh = false;
            const int rc = ws.ensure(name, bytes, &fresh);
            std::printf("%d %d", rc, (int)fresh);
        } else if (!std::strcmp(cmd, "ensure_all")) {
            int k;
            if (std::scanf("%d", &k) != 1 || k < 0 || k > 16) return 1;
            std::vector<std::string> names(k);
            std::vector<WsItem> items(k);
            for (int i = 0; i < k; ++i) {
                if (std::scanf("%63s %zu", name, &items[i].bytes) != 2) return 1;
                names[i] = name;
            }
            for (int i = 0; i < k; ++i) items[i].n = names[i].c_str();
            std::string failed = "-";
            const int rc = ws.ensure_all(items.data(), items.size(), &failed);
            std::printf("%d %s", rc, failed.c_str());
        } else if (!std::strcmp(cmd, "get")) {
            if (std::scanf("%63s", name) != 1) return 1;
            const DevBuf* b = cws.find(name);
            std::printf("%llu %zu %d %d", (unsigned long long)(uintptr_t)cws.get<char>(name), cws.bytes(name), (int)(b != nullptr),
                        (int)(b && b->p == cws.get<void>(name) && b->f() == cws.get(name)));
        } else if (!std::strcmp(cmd, "release_all")) {
            ws.release_all();
            std::printf("ok");
        } else
            return 2;
        tail();
    }
    ws.release_all();
    return g_allocs == g_frees ? 0 : 3;
}
