// carver_check.cpp -- stand-alone check of devbuf.h's Carver (plain host code, no HIP): built and run by
// tests/test_engine_layers.py with -fsanitize=address,undefined.  The layouts are the host entry points' own lists.
#define FHE_AMD_CARVER_ONLY
#include "devbuf.h"

#include <cstdio>
#include <cstring>
#include <vector>

using fhe_amd::Carver;

static int fails = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);        \
            ++fails;                                                   \
        }                                                              \
    } while (0)

template <typename F>
static bool throws_logic_error(F&& f) {
    try {
        f();
    } catch (const std::logic_error&) {
        return true;
    }
    return false;
}

// a listed layout handed out in order: consecutive, non-overlapping, inside a block of exactly words() words
static void check_layout(const std::vector<size_t>& parts) {
    Carver cv;
    size_t sum = 0;
    for (size_t w : parts) {
        cv.add(w);
        sum += w;
    }
    EXPECT(cv.words() == sum);
    std::vector<uint64_t> block(sum);  // exactly the reserved size: the sanitizer sees any write past it
    cv.bind(block.data());
    size_t off = 0;
    for (size_t i = 0; i < parts.size(); ++i) {
        uint64_t* p = cv.take(parts[i]);
        EXPECT(p == block.data() + off);
        if (parts[i]) std::memset(p, 0xA5, parts[i] * 8);  // the whole sub-array is writable
        off += parts[i];
    }
    EXPECT(off == sum);
    EXPECT(throws_logic_error([&] { cv.take(1); }));  // past the end
    EXPECT(throws_logic_error([&] { cv.take(0); }));
}

int main() {
    const size_t n = 503, N = 1024;
    for (size_t count : {(size_t)1, (size_t)5, (size_t)2}) {
        // the 2-input gate: two (a, b) columns, outputs [count][n] / [count]
        check_layout({count * n, count, count * n, count, count * n, count});
        // AND4 with ctExt left in the workspace: four columns, no staged output
        check_layout({count * n, count, count * n, count, count * n, count, count * n, count, 0, 0});
        // mixed moduli: a column of N-word rows with its flags, one of n-word rows, a ctExt-wide output
        check_layout({count * N, count, (count + 7) / 8, count * n, count, (count + 7) / 8, count * N, count});
        // public-key encryption: int32 messages in (count + 1) / 2 words
        check_layout({(count + 1) / 2, count * N, count});
    }
    check_layout({});
    {   // a request of another size than listed, or out of order, is refused and hands nothing out
        Carver cv({10, 3, 10});
        std::vector<uint64_t> block(cv.words());
        cv.bind(block.data());
        EXPECT(cv.words() == 23);
        EXPECT(throws_logic_error([&] { cv.take(11); }));
        EXPECT(throws_logic_error([&] { cv.take(3); }));
        EXPECT(cv.take(10) == block.data());
        EXPECT(cv.take(3) == block.data() + 10);
        EXPECT(throws_logic_error([&] { cv.take(3); }));
        EXPECT(cv.take(10) == block.data() + 13);
        EXPECT(throws_logic_error([&] { cv.take(10); }));
        cv.bind(block.data());  // a rebound carver starts over
        EXPECT(cv.take(10) == block.data());
    }
    if (fails) {
        std::printf("carver: %d failures\n", fails);
        return 1;
    }
    std::printf("carver ok\n");
    return 0;
}
