// C++ test of place_recognition::ScanContext / ScanContextDatabase / initial_guesses. Built and run by
// tests/test_gpu_scan_context.py on a GPU box: test_place_recognition <clouds file>; exit code 0 = all checks passed.
// The clouds file (written by that test): int32 count, then count int32 sizes | then every cloud's points (4 floats each). Cloud 0
// is the query, the others are the database's entries in order.
//   descriptors  the descriptor of every cloud; its bytes as a checksum ("F <name> <fnv1a-64>") for the Python test; a second
//                compute gives the same bytes
//   database     add(cloud) and add(descriptor) give the same candidates; query(k = 4): "C <index> <distance bits> <shift>
//                <yaw bits>", compared bit for bit with the Python mirror's; exclude_recent leaves the last entries out; a database
//                grown from capacity 1 answers alike; clear() empties it
//   guesses      initial_guesses(candidate 0, 5) as bit patterns ("T guess<i> <16 hex words>"), compared with the mirror's
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sycl_points/amd/place_recognition.hpp"

using namespace sycl_points;
namespace pr = sycl_points::algorithms::place_recognition;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("  CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static uint64_t checksum(const pr::ScanContextDescriptor& d) {
    const auto& host = d.values->host();
    uint64_t h = 1469598103934665603ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(host.data());
    for (size_t i = 0; i < host.size() * sizeof(float); ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}
static uint32_t bits(float v) {
    uint32_t w;
    std::memcpy(&w, &v, sizeof w);
    return w;
}
static bool same(const std::vector<pr::LoopCandidate>& a, const std::vector<pr::LoopCandidate>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].index != b[i].index || bits(a[i].distance) != bits(b[i].distance) || a[i].shift != b[i].shift) return false;
    return true;
}
static void section(const char* name, int failed_before) { std::printf("[ %s ] %s\n", g_failed == failed_before ? " OK " : "FAIL", name); }

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <clouds file>\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    int32_t count = 0;
    f.read(reinterpret_cast<char*>(&count), sizeof count);
    if (!f || count < 2 || count > 64) { std::printf("cannot read %s\n", argv[1]); return 2; }
    std::vector<int32_t> sizes(count);
    f.read(reinterpret_cast<char*>(sizes.data()), sizeof(int32_t) * count);
    sycl_utils::DeviceQueue queue(0);
    std::vector<PointCloudShared> clouds;
    for (int32_t c = 0; c < count; ++c) {
        PointCloudCPU cpu;
        cpu.points->resize(sizes[c]);
        f.read(reinterpret_cast<char*>(cpu.points->data()), sizeof(float) * 4 * sizes[c]);
        clouds.emplace_back(queue, cpu);
    }
    if (!f) { std::printf("%s is too short\n", argv[1]); return 2; }
    const pr::ScanContextParams params;

    int before = g_failed;
    std::vector<pr::ScanContextDescriptor> desc;
    for (int32_t c = 0; c < count; ++c) {
        desc.push_back(pr::ScanContext::compute(queue, clouds[c], params));
        const std::string name = c == 0 ? "query" : "entry" + std::to_string(c - 1);
        std::printf("F %s %016llx\n", name.c_str(), (unsigned long long)checksum(desc.back()));
        CHECK(desc.back().values->size() == size_t(params.rings) * params.sectors);
        CHECK(checksum(pr::ScanContext::compute(queue, clouds[c], params)) == checksum(desc.back()));
    }
    section("descriptors", before);

    before = g_failed;
    pr::ScanContextDatabase db(queue, params), by_descriptor(queue, params), grown(queue, params, 1);
    for (int32_t c = 1; c < count; ++c) {
        CHECK(db.add(clouds[c]) == size_t(c - 1));
        by_descriptor.add(desc[c]);
        grown.add(desc[c]);
    }
    CHECK(db.size() == size_t(count - 1) && grown.size() == db.size());
    const auto candidates = db.query(desc[0], 4);
    CHECK(candidates.size() == std::min<size_t>(4, db.size()));
    for (const auto& c : candidates) std::printf("C %d %08x %d %08x\n", c.index, bits(c.distance), c.shift, bits(c.yaw));
    CHECK(same(candidates, by_descriptor.query(desc[0], 4)) && same(candidates, grown.query(desc[0], 4)));
    CHECK(same(candidates, db.query(clouds[0], 4)));
    CHECK(db.query(desc[0], SP_SCAN_CONTEXT_MAX_K).size() == db.size() && db.query(desc[0], 4, db.size()).empty());
    for (const auto& c : db.query(desc[0], 4, 1)) CHECK(c.index >= 0 && size_t(c.index) + 1 < db.size());
    grown.clear();
    CHECK(grown.size() == 0 && grown.query(desc[0], 4).empty());
    pr::ScanContextParams other = params;
    other.sectors = 30;
    bool threw = false;
    try { db.add(pr::ScanContext::compute(queue, clouds[0], other)); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
    section("database", before);

    before = g_failed;
    if (!candidates.empty()) {
        const auto guesses = pr::initial_guesses(candidates[0], 5);
        CHECK(guesses.size() == 5);
        for (size_t i = 0; i < guesses.size(); ++i) {
            std::printf("T guess%zu", i);
            for (int e = 0; e < 16; ++e) std::printf(" %08x", bits(guesses[i].data()[e]));
            std::printf("\n");
            CHECK(guesses[i](3, 3) == 1.0f && guesses[i](0, 3) == 0.0f && guesses[i](2, 2) == 1.0f);
        }
        CHECK(pr::initial_guesses(candidates[0], 1).size() == 1 && pr::initial_guesses(candidates[0], 0).empty());
    }
    section("guesses", before);

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
