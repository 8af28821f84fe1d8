// scripts/draw_host_sanitize.cpp -- the host-only pieces of the device episode generators under AddressSanitizer and UBSan (scripts/draw_host_sanitize.sh
// builds and runs it; no GPU involved): the table of draw kinds, the generic host hook and the host twins behind it, for one scenario of every kind and for
// one the table refuses.
#include <cctype>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/megaverse_hip.h"

// what the hooks take from mv_api.hip, which is not part of this program
namespace mvapi {
thread_local std::string g_err;
std::string lower(const char *s)
{
    std::string r(s);
    for (auto &c : r) c = (char)std::tolower((unsigned char)c);
    return r;
}
}  // namespace mvapi

int main()
{
    int bad = 0;
    for (const char *name : {"Collect", "ObstaclesHard", "Empty", "HexMemory"}) {
        const int size = mv_debug_draw_host(name, 1, 0, 1, 60.0f, nullptr, 0);
        if (size <= 0) { std::printf("%s: no record size (%s)\n", name, mvapi::g_err.c_str()); return 1; }
        std::vector<unsigned char> record((size_t)size);   // (exactly the record: a byte past it is the sanitizer's)
        int episodes = 0;
        for (int agents : {1, 2, 8})
            for (int seed : {0, 1, 42, 28, (1 << 30) - 1})
                for (int n : {1, 2, 3}) {
                    if (mv_debug_draw_host(name, agents, seed, n, 60.0f, record.data(), size) != size) { std::printf("%s: %s\n", name, mvapi::g_err.c_str()); ++bad; }
                    int seq;
                    std::memcpy(&seq, record.data(), sizeof seq);
                    if (seq != n) { std::printf("%s: seq %d, not %d\n", name, seq, n); ++bad; }
                    ++episodes;
                }
        if (mv_debug_draw_host(name, 1, 0, 1, 60.0f, record.data(), size - 1) != -1) { std::printf("%s: a short buffer was taken\n", name); ++bad; }
        std::printf("%s: %d episodes, record of %d bytes\n", name, episodes, size);
    }
    if (mv_debug_draw_host("Rearrange", 1, 0, 1, 60.0f, nullptr, 0) != -1) { std::printf("Rearrange was not refused\n"); ++bad; }
    std::printf("Rearrange: %s\n", mvapi::g_err.c_str());
    std::printf(bad ? "FAILED\n" : "clean\n");
    return bad ? 1 : 0;
}
