// s2s_host.cpp -- host-side (no GPU) helpers of the predict path's back end, part of libs2s_hip.so.
//
// s2s_blow5_pack frames and compresses one batch of BLOW5 records on worker threads: the job pyslow5's
// write_record_batch(threads = cpu_count) does for the reference (signal_io.py:167-171).  The Python writer builds the small
// per-record field bytes (ids, calibration, auxiliary fields -- signal_io.py:143-161) and hands over the packed int16 samples
// as they came off the GPU; nothing here runs under the interpreter lock.
#include "../../include/s2s_hip.h"
#include "s2s_event_fixed.h"

#include <dlfcn.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace {

// ---- optional codecs, bound at first use (neither ships a header in this image)
struct Zstd {
    size_t (*compress)(void*, size_t, const void*, size_t, int) = nullptr;
    size_t (*bound)(size_t) = nullptr;
    unsigned (*is_error)(size_t) = nullptr;
    bool ok = false;
    Zstd() {
        void* h = dlopen("libzstd.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        compress = reinterpret_cast<decltype(compress)>(dlsym(h, "ZSTD_compress"));
        bound = reinterpret_cast<decltype(bound)>(dlsym(h, "ZSTD_compressBound"));
        is_error = reinterpret_cast<decltype(is_error)>(dlsym(h, "ZSTD_isError"));
        ok = compress && bound && is_error;
    }
};
const Zstd& zstd() { static Zstd z; return z; }

// libdeflate writes the same zlib container (RFC 1950) about three times faster than zlib's own level 1
struct Deflate {
    void* (*alloc)(int) = nullptr;
    size_t (*zlib_compress)(void*, const void*, size_t, void*, size_t) = nullptr;
    size_t (*zlib_bound)(void*, size_t) = nullptr;
    void (*free_)(void*) = nullptr;
    bool ok = false;
    Deflate() {
        void* h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        alloc = reinterpret_cast<decltype(alloc)>(dlsym(h, "libdeflate_alloc_compressor"));
        zlib_compress = reinterpret_cast<decltype(zlib_compress)>(dlsym(h, "libdeflate_zlib_compress"));
        zlib_bound = reinterpret_cast<decltype(zlib_bound)>(dlsym(h, "libdeflate_zlib_compress_bound"));
        free_ = reinterpret_cast<decltype(free_)>(dlsym(h, "libdeflate_free_compressor"));
        ok = alloc && zlib_compress && zlib_bound && free_;
    }
};
const Deflate& deflate() { static Deflate d; return d; }

// ---- a process-wide pool of worker threads; run(n, fn) calls fn(i, worker) for i in [0, n) and returns when all are done
class Pool {
  public:
    explicit Pool(int n) {
        for (int w = 0; w < n; ++w) workers_.emplace_back([this, w] { loop(w); });
    }
    ~Pool() {
        { std::lock_guard<std::mutex> l(m_); stop_ = true; }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }
    int size() const { return (int)workers_.size(); }
    void run(int n, const std::function<void(int, int)>& fn) {
        std::unique_lock<std::mutex> l(m_);
        fn_ = &fn; n_ = n; next_ = 0; left_ = n; ++gen_;
        cv_.notify_all();
        // every task done AND every worker that joined this generation back out of its task loop: none of them may
        // touch `fn` or the task counter of the next call
        done_.wait(l, [this] { return left_ == 0 && active_ == 0; });
        fn_ = nullptr;
    }

  private:
    void loop(int w) {
        unsigned long seen = 0;
        for (;;) {
            const std::function<void(int, int)>* fn;
            int n;
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [&] { return stop_ || (gen_ != seen && fn_); });
                if (stop_) return;
                seen = gen_;
                fn = fn_;
                n = n_;
                ++active_;
            }
            int finished = 0;
            for (;;) {
                const int i = next_.fetch_add(1);
                if (i >= n) break;
                (*fn)(i, w);
                ++finished;
            }
            std::lock_guard<std::mutex> l(m_);
            left_ -= finished;
            --active_;
            if (left_ == 0 && active_ == 0) done_.notify_all();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(int, int)>* fn_ = nullptr;
    std::atomic<int> next_{0};
    int n_ = 0, left_ = 0, active_ = 0;
    unsigned long gen_ = 0;
    bool stop_ = false;
};

std::mutex g_pool_mutex;          // one batch at a time (the writers call from a single writer thread anyway)
Pool* g_pool = nullptr;
std::vector<std::vector<uint8_t>> g_scratch;   // per worker: the uncompressed body of the record it is on (kept between calls:
                                               // fresh pages every batch cost more than the compression of a small one)

// ---- Huffman-only deflate (RFC 1951, dynamic blocks, literals only): the encoder of method 3.
// A nanopore signal is noise on top of a level: LZ77 finds next to nothing in it (libdeflate level 1: 0.69-0.77 of the raw size,
// Huffman coding of the bytes alone: 0.71-0.78), but the match search is what a deflate encoder spends its time in.  One piece =
// one dynamic block with its own code + an empty stored block that pads to a byte boundary (and carries the final bit of the
// last piece), so pieces are encoded independently and laid back to back.

// Code lengths (<= max_len, a complete code) for freq[0..n): symbols with freq 0 get length 0; at least two symbols get a code.
void huff_lengths(const uint32_t* freq_in, int n, int max_len, uint8_t* len_out) {
    uint32_t freq[288];
    int order[288], used = 0;
    for (int i = 0; i < n; ++i) { freq[i] = freq_in[i]; len_out[i] = 0; }
    for (int i = 0; i < n && used < 2; ++i) used += freq[i] != 0;
    for (int i = 0; used < 2; ++i)                       // a decoder wants a complete code: give a second symbol a leaf
        if (!freq[i]) { freq[i] = 1; ++used; }
    used = 0;
    for (int i = 0; i < n; ++i)
        if (freq[i]) order[used++] = i;
    std::sort(order, order + used, [&](int a, int b) { return freq[a] != freq[b] ? freq[a] < freq[b] : a < b; });
    // two-queue Huffman: leaves in ascending order, internal nodes are created in ascending order as well
    uint64_t w[576];
    int parent[576];
    for (int i = 0; i < used; ++i) w[i] = freq[order[i]];
    int leaf = 0, inner = used, made = used;
    auto take = [&]() { return (leaf < used && (inner >= made || w[leaf] <= w[inner])) ? leaf++ : inner++; };
    while (made < 2 * used - 1) {
        const int a = take(), b = take();
        w[made] = w[a] + w[b];
        parent[a] = parent[b] = made;
        ++made;
    }
    int count[64] = {0};
    for (int i = 0; i < used; ++i) {
        int d = 0;
        for (int v = i; v != made - 1; v = parent[v]) ++d;
        ++count[d < 63 ? d : 63];
    }
    // enforce max_len: everything deeper moves up to max_len, then lengths are traded until the Kraft sum is exactly one
    for (int d = max_len + 1; d < 64; ++d) { count[max_len] += count[d]; count[d] = 0; }
    uint64_t total = 0;
    for (int d = 1; d <= max_len; ++d) total += (uint64_t)count[d] << (max_len - d);
    while (total > (1ull << max_len)) {
        --count[max_len];
        for (int d = max_len - 1; d > 0; --d)
            if (count[d]) { --count[d]; count[d + 1] += 2; break; }
        --total;
    }
    int at = 0;                                          // rarest symbols take the longest codes
    for (int d = max_len; d >= 1; --d)
        for (int c = 0; c < count[d]; ++c) len_out[order[at++]] = (uint8_t)d;
}

// canonical codes of the lengths, bit-reversed (deflate writes Huffman codes starting from their most significant bit)
void huff_codes(const uint8_t* len, int n, uint16_t* code) {
    int bl_count[16] = {0}, next[16];
    for (int i = 0; i < n; ++i) ++bl_count[len[i]];
    bl_count[0] = 0;
    int c = 0;
    for (int b = 1; b < 16; ++b) { c = (c + bl_count[b - 1]) << 1; next[b] = c; }
    for (int i = 0; i < n; ++i) {
        if (!len[i]) { code[i] = 0; continue; }
        unsigned v = (unsigned)next[len[i]]++, r = 0;
        for (int b = 0; b < len[i]; ++b) { r = (r << 1) | (v & 1); v >>= 1; }
        code[i] = (uint16_t)r;
    }
}

struct BitOut {
    uint8_t* p;
    uint64_t acc = 0;
    int n = 0;
    explicit BitOut(uint8_t* dst) : p(dst) {}
    inline void put(uint32_t v, int bits) {              // bits <= 30; the buffer holds < 32 bits on entry
        acc |= (uint64_t)v << n;
        n += bits;
        if (n >= 32) { std::memcpy(p, &acc, 4); p += 4; acc >>= 32; n -= 32; }      // (little-endian host)
    }
    // Four codes of <= 15 bits each behind < 8 pending bits: one unconditional 8-byte store, the pointer moves by the whole bytes
    // (the destination has slack behind the stream: see the bound at huff_deflate_piece).
    inline void put4(uint32_t a, int la, uint32_t b, int lb, uint32_t c, int lc, uint32_t d, int ld) {
        if (n + la + lb + lc + ld >= 64) {               // four long codes in a row (rare symbols): the 64-bit word would overflow
            put(a | b << la, la + lb);
            put(c | d << lc, lc + ld);
            align_pending();
            return;
        }
        uint64_t v = acc | (uint64_t)a << n;
        int m = n + la;
        v |= (uint64_t)b << m; m += lb;
        v |= (uint64_t)c << m; m += lc;
        v |= (uint64_t)d << m; m += ld;                  // m < 64
        std::memcpy(p, &v, 8);
        p += m >> 3;
        acc = v >> (m & ~7);
        n = m & 7;
    }
    inline void align_pending() {                        // bring the buffer below 8 pending bits (put4's entry condition)
        while (n >= 8) { *p++ = (uint8_t)acc; acc >>= 8; n -= 8; }
    }
    uint8_t* finish() {                                  // pad to a byte boundary
        while (n > 0) { *p++ = (uint8_t)acc; acc >>= 8; n -= 8; }
        n = 0; acc = 0;
        return p;
    }
};

struct Segs {                                            // bytes [lo, hi) of the concatenation of up to three buffers
    const uint8_t* p[3];
    int64_t n[3];
    template <class F> void each(int64_t lo, int64_t hi, F&& f) const {
        int64_t base = 0;
        for (int s = 0; s < 3; ++s) {
            const int64_t a = lo > base ? lo : base, b = hi < base + n[s] ? hi : base + n[s];
            if (b > a) f(p[s] + (a - base), b - a);
            base += n[s];
        }
    }
};

// One piece -> dst (room >= len + len / 128 + 512): [dynamic block | stored blocks when those are smaller][empty stored block,
// final bit = last].  Returns the bytes written; *adler = Adler-32 of the piece's bytes.
int64_t huff_deflate_piece(const Segs& in, int64_t lo, int64_t hi, bool last, uint8_t* dst, uint32_t* adler) {
    uint32_t hist[8][256];                               // eight tables: int16 samples put near-equal bytes two apart
    std::memset(hist, 0, sizeof hist);
    uint32_t ad = 1;
    in.each(lo, hi, [&](const uint8_t* s, int64_t m) {
        ad = (uint32_t)adler32(ad, s, (uInt)m);
        int64_t i = 0;
        for (; i + 8 <= m; i += 8) {
            uint64_t w;
            std::memcpy(&w, s + i, 8);
            ++hist[0][w & 255]; ++hist[1][(w >> 8) & 255]; ++hist[2][(w >> 16) & 255]; ++hist[3][(w >> 24) & 255];
            ++hist[4][(w >> 32) & 255]; ++hist[5][(w >> 40) & 255]; ++hist[6][(w >> 48) & 255]; ++hist[7][w >> 56];
        }
        for (; i < m; ++i) ++hist[0][s[i]];
    });
    *adler = ad;
    uint32_t freq[257];
    for (int i = 0; i < 256; ++i) {
        freq[i] = 0;
        for (int k = 0; k < 8; ++k) freq[i] += hist[k][i];
    }
    freq[256] = 1;                                       // end of block
    uint8_t len[259];
    huff_lengths(freq, 257, 15, len);
    len[257] = len[258] = 1;                             // two distance codes of one bit, never used (what zlib sends as well)
    uint32_t clfreq[19] = {0};
    for (int i = 0; i < 259; ++i) ++clfreq[len[i]];
    uint8_t cllen[19];
    huff_lengths(clfreq, 16, 7, cllen);
    cllen[16] = cllen[17] = cllen[18] = 0;               // the run-length symbols are not used: 259 lengths cost ~130 bytes
    uint16_t code[257], clcode[19];
    huff_codes(len, 257, code);
    huff_codes(cllen, 19, clcode);
    int64_t bits = 3 + 5 + 5 + 4 + 19 * 3;
    for (int i = 0; i < 259; ++i) bits += cllen[len[i]];
    for (int i = 0; i < 257; ++i) bits += (int64_t)freq[i] * len[i];
    const int64_t n = hi - lo;
    uint8_t* p = dst;
    if ((bits + 7) / 8 >= n + 5 * ((n + 65534) / 65535)) {
        // incompressible: stored blocks (byte-aligned by construction)
        int64_t at = lo;
        while (at < hi) {
            const int64_t m = hi - at < 65535 ? hi - at : 65535;
            *p++ = 0;
            *p++ = (uint8_t)m; *p++ = (uint8_t)(m >> 8); *p++ = (uint8_t)~m; *p++ = (uint8_t)(~m >> 8);
            in.each(at, at + m, [&](const uint8_t* s, int64_t k) { std::memcpy(p, s, k); p += k; });
            at += m;
        }
    } else {
        BitOut out(p);
        out.put(0, 1);                                   // not the final block: the empty stored block below carries that bit
        out.put(2, 2);                                   // dynamic Huffman codes
        out.put(0, 5);                                   // HLIT: 257 literal/length codes
        out.put(1, 5);                                   // HDIST: 2 distance codes
        out.put(15, 4);                                  // HCLEN: all 19 code length codes
        static const uint8_t cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (int i = 0; i < 19; ++i) out.put(cllen[cl_order[i]], 3);
        for (int i = 0; i < 259; ++i) out.put(clcode[len[i]], cllen[len[i]]);
        uint32_t tab[256];                               // code | length << 16
        for (int i = 0; i < 256; ++i) tab[i] = code[i] | (uint32_t)len[i] << 16;
        in.each(lo, hi, [&](const uint8_t* s, int64_t m) {
            int64_t i = 0;
            out.align_pending();
            for (; i + 4 <= m; i += 4) {                 // four codes (<= 15 bits each) per store
                const uint32_t t = tab[s[i]], u = tab[s[i + 1]], v = tab[s[i + 2]], w = tab[s[i + 3]];
                out.put4(t & 0xFFFF, (int)(t >> 16), u & 0xFFFF, (int)(u >> 16), v & 0xFFFF, (int)(v >> 16), w & 0xFFFF, (int)(w >> 16));
            }
            for (; i < m; ++i) { const uint32_t t = tab[s[i]]; out.put(t & 0xFFFF, (int)(t >> 16)); }
        });
        out.put(code[256], len[256]);
        out.put(last ? 1 : 0, 1);                        // the empty stored block: final bit, type 00, pad, LEN 0, NLEN ~0
        out.put(0, 2);
        p = out.finish();
        *p++ = 0; *p++ = 0; *p++ = 0xFF; *p++ = 0xFF;
        return p - dst;
    }
    *p++ = last ? 1 : 0;                                 // after stored blocks the stream is byte-aligned already
    *p++ = 0; *p++ = 0; *p++ = 0xFF; *p++ = 0xFF;
    return p - dst;
}

}  // namespace

extern "C" {

int64_t s2s_blow5_pack_bound(int64_t body_bytes_total, int32_t n_records) {
    if (body_bytes_total < 0 || n_records < 0) return S2S_ERR_ARG;
    // per record: u64 size + the worst case of the three codecs (zstd's bound is the largest: n + n/256 + 64); a long zlib
    // record's pieces each end in a flush marker
    return body_bytes_total + body_bytes_total / 64 + (int64_t)n_records * (8 + 1024) + 4096;
}

int64_t s2s_blow5_pack(const uint8_t* prefix, const int64_t* prefix_offs, const uint8_t* suffix, const int64_t* suffix_offs,
                       const uint8_t* signal, const int64_t* signal_offs, int32_t n, int32_t method, int32_t level,
                       int32_t threads, uint8_t* out, int64_t capacity) {
    if (n < 0 || threads < 1 || (n > 0 && (!prefix || !prefix_offs || !suffix || !suffix_offs || !signal || !signal_offs || !out)))
        return S2S_ERR_ARG;
    if (method < 0 || method > 3) return S2S_ERR_ARG;
    if (method == 2 && !zstd().ok) return S2S_ERR_CODEC;
    if (n == 0) return 0;
    std::lock_guard<std::mutex> guard(g_pool_mutex);
    if (!g_pool || g_pool->size() < threads) { delete g_pool; g_pool = new Pool(threads); }   // grows, never shrinks
    const int workers = g_pool->size();
    const int zlevel = level < 1 ? 1 : (level > 9 ? 9 : level);

    // One task per record -- except that a batch is only done when its longest record is: with method 3 a record is deflated
    // as independent pieces of at most PIECE bytes (huff_deflate_piece); header + pieces + Adler-32 of the whole body are one
    // ordinary zlib stream (RFC 1950).
    constexpr int64_t PIECE = 128 << 10;
    struct Task { int rec; int64_t lo, hi; bool piece, last; int64_t slot, room, size; uint32_t adler; };
    std::vector<Task> tasks;
    std::vector<int> first_task(n + 1);
    int64_t need = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t body = (prefix_offs[i + 1] - prefix_offs[i]) + (signal_offs[i + 1] - signal_offs[i]) + (suffix_offs[i + 1] - suffix_offs[i]);
        first_task[i] = (int)tasks.size();
        if (method == 3) {
            const int64_t k = body > 0 ? (body + PIECE - 1) / PIECE : 1, len = body > 0 ? (body + k - 1) / k : 1;
            for (int64_t lo = 0; lo < body || lo == 0; lo += len) {
                const int64_t hi = lo + len < body ? lo + len : body;
                const int64_t room = (hi - lo) + (hi - lo) / 128 + 512;
                tasks.push_back({i, lo, hi, true, hi == body, need, room, 0, 0});
                need += room;
            }
        } else {
            const int64_t room = body + body / 128 + 1024;
            tasks.push_back({i, 0, body, false, true, need, room, 0, 0});
            need += room;
        }
    }
    first_task[n] = (int)tasks.size();
    static std::vector<uint8_t> staged;            // compressed pieces before they are laid back to back (kept between calls)
    if ((int64_t)staged.size() < need) staged.resize(need + need / 4);
    std::atomic<int> failed{0};
    if ((int)g_scratch.size() < workers) g_scratch.resize(workers);
    std::vector<std::vector<uint8_t>>& scratch = g_scratch;
    std::vector<void*> defl(workers, nullptr);
    const bool use_deflate = method == 1 && deflate().ok;
    g_pool->run((int)tasks.size(), [&](int t, int w) {
        Task& T = tasks[t];
        const int i = T.rec;
        const int64_t np = prefix_offs[i + 1] - prefix_offs[i], ns = signal_offs[i + 1] - signal_offs[i], nx = suffix_offs[i + 1] - suffix_offs[i];
        const int64_t body = np + ns + nx;
        uint8_t* dst = staged.data() + T.slot;
        int64_t written = -1;
        if (T.piece) {
            const Segs in = {{prefix + prefix_offs[i], signal + signal_offs[i], suffix + suffix_offs[i]}, {np, ns, nx}};
            written = huff_deflate_piece(in, T.lo, T.hi, T.last, dst, &T.adler);
            if (written > T.room) written = -1;
        } else if (method == 0) {
            std::memcpy(dst, prefix + prefix_offs[i], np);
            std::memcpy(dst + np, signal + signal_offs[i], ns);
            std::memcpy(dst + np + ns, suffix + suffix_offs[i], nx);
            written = body;
        } else {
            std::vector<uint8_t>& b = scratch[w];
            if ((int64_t)b.size() < body) b.resize(body);
            std::memcpy(b.data(), prefix + prefix_offs[i], np);
            std::memcpy(b.data() + np, signal + signal_offs[i], ns);
            std::memcpy(b.data() + np + ns, suffix + suffix_offs[i], nx);
            if (use_deflate) {
                if (!defl[w]) defl[w] = deflate().alloc(zlevel);
                const size_t r = defl[w] ? deflate().zlib_compress(defl[w], b.data(), body, dst, T.room) : 0;
                if (r) written = (int64_t)r;
            } else if (method == 1) {
                uLongf dl = (uLongf)T.room;
                if (compress2(dst, &dl, b.data(), (uLong)body, level) == Z_OK) written = (int64_t)dl;
            } else {
                const size_t r = zstd().compress(dst, T.room, b.data(), body, level);
                if (!zstd().is_error(r)) written = (int64_t)r;
            }
        }
        if (written < 0) { failed = 1; written = 0; }
        T.size = written;
    });
    for (void* d : defl)
        if (d) deflate().free_(d);
    if (failed) return S2S_ERR_CODEC;

    // where every record lands in `out`, then the copies (again on the workers: 10+ MB per batch)
    std::vector<int64_t> at(n + 1);
    at[0] = 0;
    for (int i = 0; i < n; ++i) {
        int64_t len = 0;
        for (int t = first_task[i]; t < first_task[i + 1]; ++t) len += tasks[t].size;
        if (tasks[first_task[i]].piece) len += 2 + 4;
        at[i + 1] = at[i] + 8 + len;
    }
    if (at[n] > capacity) return S2S_ERR_ARG;
    g_pool->run(n, [&](int i, int) {
        uint8_t* dst = out + at[i];
        const uint64_t sz = (uint64_t)(at[i + 1] - at[i] - 8);
        std::memcpy(dst, &sz, 8);                               // (little-endian host)
        dst += 8;
        const bool split = tasks[first_task[i]].piece;
        uint32_t ad = 1;
        if (split) { *dst++ = 0x78; *dst++ = 0x01; }             // CMF/FLG: deflate, 32 K window, fastest, check bits
        for (int t = first_task[i]; t < first_task[i + 1]; ++t) {
            const Task& T = tasks[t];
            std::memcpy(dst, staged.data() + T.slot, T.size);
            dst += T.size;
            if (split) ad = t == first_task[i] ? T.adler : (uint32_t)adler32_combine(ad, T.adler, (z_off_t)(T.hi - T.lo));
        }
        if (split) { dst[0] = (uint8_t)(ad >> 24); dst[1] = (uint8_t)(ad >> 16); dst[2] = (uint8_t)(ad >> 8); dst[3] = (uint8_t)ad; }
    });
    return at[n];
}

int64_t s2s_compress_rows(const uint8_t* in, const int64_t* in_offs, int32_t n, int32_t method, int32_t level, int32_t threads,
                          uint8_t* out, int64_t capacity, int64_t* out_offs) {
    if (n < 0 || threads < 1 || !out_offs || (n > 0 && (!in || !in_offs || !out))) return S2S_ERR_ARG;
    if (method != 1 && method != 2) return S2S_ERR_ARG;
    if (method == 2 && !zstd().ok) return S2S_ERR_CODEC;
    out_offs[0] = 0;
    if (n == 0) return 0;
    std::lock_guard<std::mutex> guard(g_pool_mutex);
    if (!g_pool || g_pool->size() < threads) { delete g_pool; g_pool = new Pool(threads); }
    const int workers = g_pool->size();
    std::vector<int64_t> slot(n + 1), size(n);
    slot[0] = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t len = in_offs[i + 1] - in_offs[i];
        if (len < 0) return S2S_ERR_ARG;
        slot[i + 1] = slot[i] + len + len / 128 + 1024;
    }
    if (slot[n] > capacity) return S2S_ERR_ARG;
    std::atomic<int> failed{0};
    std::vector<void*> defl(workers, nullptr);
    const bool use_deflate = method == 1 && deflate().ok;
    g_pool->run(n, [&](int i, int w) {
        const uint8_t* src = in + in_offs[i];
        const int64_t len = in_offs[i + 1] - in_offs[i], room = slot[i + 1] - slot[i];
        uint8_t* dst = out + slot[i];
        int64_t written = -1;
        if (use_deflate) {
            if (!defl[w]) defl[w] = deflate().alloc(level < 1 ? 1 : level);
            const size_t r = defl[w] ? deflate().zlib_compress(defl[w], src, len, dst, room) : 0;
            if (r) written = (int64_t)r;
        } else if (method == 1) {
            uLongf dl = (uLongf)room;
            if (compress2(dst, &dl, src, (uLong)len, level) == Z_OK) written = (int64_t)dl;
        } else {
            const size_t r = zstd().compress(dst, room, src, len, level);
            if (!zstd().is_error(r)) written = (int64_t)r;
        }
        if (written < 0) { failed = 1; written = 0; }
        size[i] = written;
    });
    for (void* d : defl)
        if (d) deflate().free_(d);
    if (failed) return S2S_ERR_CODEC;
    int64_t pos = 0;
    for (int i = 0; i < n; ++i) {                               // close the gaps, in row order
        if (pos != slot[i]) std::memmove(out + pos, out + slot[i], size[i]);
        pos += size[i];
        out_offs[i + 1] = pos;
    }
    return pos;
}

}  // extern "C"

// ================================================================================ base-to-signal alignment (PAF)
// One line per record of the signal file from the per-chunk counts of s2s_align_chunks.  A read is a walk over events in the
// order of its STORED signal: per chunk its te k-mer segments (a real k-mer while fewer than K have been seen, else a pad k-mer of
// the last chunk: an insertion) and then the chunk's tail (an insertion); an RNA read is stored reversed, so its walk runs
// backwards.  Insertions in front of the first and behind the last real k-mer are trimmed into sig_start / sig_end.
namespace {

inline uint8_t* put_u64(uint8_t* p, uint64_t v) {
    char tmp[20];
    int n = 0;
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) *p++ = (uint8_t)tmp[--n];
    return p;
}

// bytes one read's line may take: <= 6 per event (any uint16 count and its letter: "65535,"; a merged run of m insertions or of m
// empty k-mers never needs more than 6 m) + the fixed columns (seven numbers of <= 20 digits, tabs, "+", "255", "ss:Z:", the line end)
inline int64_t paf_line_bound(int64_t chunks, int32_t te, int64_t id_len) { return 6 * chunks * (te + 1) + 2 * id_len + 256; }

}  // namespace

extern "C" int64_t s2s_paf_format_bound(int64_t n_chunks, int32_t te, int32_t n_reads, int64_t id_bytes_total) {
    if (n_chunks < 0 || te < 1 || n_reads < 0 || id_bytes_total < 0) return S2S_ERR_ARG;
    return 6 * n_chunks * (te + 1) + 2 * id_bytes_total + (int64_t)n_reads * 256;
}

extern "C" int64_t s2s_paf_format(const uint16_t* seg, int32_t te, const int32_t* read_first, const int64_t* read_kmers,
                                  const int64_t* read_offs, int32_t R, const uint8_t* ids, const int64_t* id_offs, int32_t n_ids,
                                  int32_t rna, int32_t threads, uint8_t* out, int64_t capacity) {
    if (R < 0 || n_ids < 0 || te < 1 || threads < 1 || capacity < 0) return S2S_ERR_ARG;
    if (R == 0) return n_ids == 0 ? 0 : S2S_ERR_ARG;
    if (!seg || !read_first || !read_kmers || !read_offs || !id_offs || !out || (n_ids > 0 && !ids)) return S2S_ERR_ARG;
    // the records of the signal file are the reads with samples, in read order: read r's id is the next unused one
    std::vector<int32_t> id_of(R);
    std::vector<int64_t> slot(R + 1), size(R, 0);
    int32_t used = 0;
    slot[0] = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t chunks = (int64_t)read_first[r + 1] - read_first[r], n = read_offs[r + 1] - read_offs[r];
        if (chunks < 0 || n < 0 || read_kmers[r] < 0 || read_kmers[r] > chunks * te) return S2S_ERR_ARG;
        id_of[r] = -1;
        slot[r + 1] = slot[r];
        if (n == 0) continue;                                    // no samples: no record, no line
        if (used >= n_ids || id_offs[used + 1] < id_offs[used] || read_kmers[r] < 1) return S2S_ERR_ARG;
        id_of[r] = used++;
        slot[r + 1] += paf_line_bound(chunks, te, id_offs[used] - id_offs[used - 1]);
    }
    if (used != n_ids || slot[R] > capacity) return S2S_ERR_ARG;
    std::atomic<int> failed{0};
    {
        std::lock_guard<std::mutex> guard(g_pool_mutex);
        if (!g_pool || g_pool->size() < threads) { delete g_pool; g_pool = new Pool(threads); }
        g_pool->run(R, [&](int r, int) {
            if (id_of[r] < 0) return;
            const int64_t b0 = read_first[r], chunks = (int64_t)read_first[r + 1] - b0, n_ev = chunks * (te + 1);
            const int64_t K = read_kmers[r], len = read_offs[r + 1] - read_offs[r];
            // event e of the forward walk: chunk e / (te+1), slot e % (te+1); a k-mer when slot < te and chunk * te + slot < K
            auto count = [&](int64_t e) { return (int64_t)seg[(b0 + e / (te + 1)) * (te + 1) + e % (te + 1)]; };
            auto is_kmer = [&](int64_t e) { const int64_t j = e % (te + 1); return j < te && (e / (te + 1)) * te + j < K; };
            // forward event 0 is k-mer 0 and e_last the last real k-mer (K >= 1): what lies behind it is trimmed
            const int64_t e_last = ((K - 1) / te) * (te + 1) + (K - 1) % te;
            int64_t lead = 0, trail = 0, total = 0, mapped = 0;
            for (int64_t e = 0; e < n_ev; ++e) {
                const int64_t c = count(e);
                total += c;
                if (e > e_last) trail += c;
                else if (c && is_kmer(e)) ++mapped;
            }
            if (total != len) { failed = 1; return; }            // seg and the export's offsets describe different signals
            if (rna) std::swap(lead, trail);
            uint8_t* p = out + slot[r];
            const uint8_t* id = ids + id_offs[id_of[r]];
            const int64_t id_len = id_offs[id_of[r] + 1] - id_offs[id_of[r]];
            auto tab = [&] { *p++ = '\t'; };
            std::memcpy(p, id, id_len); p += id_len; tab();
            p = put_u64(p, len); tab();
            p = put_u64(p, lead); tab();
            p = put_u64(p, len - trail); tab();
            *p++ = '+'; tab();
            std::memcpy(p, id, id_len); p += id_len; tab();
            p = put_u64(p, K); tab();
            p = put_u64(p, rna ? K : 0); tab();
            p = put_u64(p, rna ? 0 : K); tab();
            p = put_u64(p, mapped); tab();
            p = put_u64(p, K); tab();
            std::memcpy(p, "255\tss:Z:", 9); p += 9;
            int64_t run_d = 0, run_i = 0;
            for (int64_t s = 0; s <= e_last; ++s) {
                const int64_t e = rna ? e_last - s : s, c = count(e);
                if (is_kmer(e)) {
                    if (run_i) { p = put_u64(p, run_i); *p++ = 'I'; run_i = 0; }
                    if (c) {
                        if (run_d) { p = put_u64(p, run_d); *p++ = 'D'; run_d = 0; }
                        p = put_u64(p, c); *p++ = ',';
                    } else {
                        ++run_d;
                    }
                } else if (c) {
                    if (run_d) { p = put_u64(p, run_d); *p++ = 'D'; run_d = 0; }
                    run_i += c;
                }
            }
            if (run_d) { p = put_u64(p, run_d); *p++ = 'D'; }      // (the walk ends on a k-mer: no insertion is pending)
            *p++ = '\n';
            size[r] = p - (out + slot[r]);
            if (size[r] > slot[r + 1] - slot[r]) failed = 1;     // (cannot happen with paf_line_bound)
        });
    }
    if (failed) return S2S_ERR_ARG;
    int64_t pos = 0;
    for (int r = 0; r < R; ++r) {                               // close the gaps, in read order
        if (size[r] && pos != slot[r]) std::memmove(out + pos, out + slot[r], size[r]);
        pos += size[r];
    }
    return pos;
}

// ================================================================================ per-k-mer event table (predict --events)
// One row per real k-mer with samples, from the counts and integer sums of s2s_event_stats; include/s2s_hip.h states the columns.
// The walk over a read's events is s2s_paf_format's: per chunk te k-mer slots, then the tail; the cursor advances over every slot,
// a row is written for a slot that is a real k-mer and holds samples.
namespace {

constexpr char kEventsHeader[] = "read_name\tposition\tmodel_kmer\tstart_idx\tend_idx\tevent_level_mean\tevent_stdv";

inline int dec_digits(uint64_t v) { int n = 1; while (v >= 10) { v /= 10; ++n; } return n; }

// Widths the numbers of a table can take with this calibration.  Every level is (x + offset) * range / digitisation with |x| <=
// 32768, every deviation at most 32768 * |range / digitisation|: none exceeds M in magnitude (the 1 + 1e-9 covers the roundings).
struct EventWidths {
    bool ok;
    int level;      // a "%.4f" column: sign, integer digits, point, four decimals
    int sample;     // a "%.3f" sample and the comma (or tab, or line end) after it
};
inline EventWidths event_widths(double dig, double range, double offset) {
    EventWidths w{false, 0, 0};
    if (!(dig == dig) || !(range == range) || !(offset == offset) || dig == 0.0 || range == 0.0) return w;
    const double M = (32768.0 + std::fabs(offset)) * std::fabs(range) / std::fabs(dig) * (1.0 + 1e-9) + 1.0;
    char tmp[400];
    const int digits = (M < 1e300) ? std::snprintf(tmp, sizeof tmp, "%.0f", M) : 312;    // (inf prints shorter than this)
    w.ok = true;
    w.level = 1 + digits + 5;
    w.sample = 1 + digits + 4 + 1;
    return w;
}

// bytes the rows of one read may take: `rows` rows of id, position, k-mer, two indices (each <= idx_digits digits), two levels, the
// seven separators and the line end, and `samples` sample fields
inline int64_t event_rows_bound(int64_t rows, int64_t id_len, int32_t k, int idx_digits, const EventWidths& w, int64_t samples) {
    return rows * (id_len + k + 3 * (int64_t)idx_digits + 2 * (int64_t)w.level + 8) + samples * w.sample;
}

}  // namespace

extern "C" int64_t s2s_events_format_bound(int64_t n_chunks, int32_t te, int64_t id_len_max, int32_t k, float digitisation, float range,
                                           float offset, int64_t n_samples, int32_t with_header) {
    const EventWidths w = event_widths(digitisation, range, offset);
    if (n_chunks < 0 || te < 1 || id_len_max < 0 || k < 1 || n_samples < 0 || !w.ok) return S2S_ERR_ARG;
    const int idx_digits = dec_digits((uint64_t)n_chunks * (uint64_t)(te + 1) * 65535u);
    return (with_header ? (int64_t)sizeof kEventsHeader + 16 : 0) + event_rows_bound(n_chunks * te, id_len_max, k, idx_digits, w, n_samples);
}

extern "C" int64_t s2s_events_format(const uint16_t* seg, const int32_t* sum, const int64_t* sumsq, int32_t te, const int32_t* read_first,
                                     const int64_t* read_kmers, const int64_t* read_offs, int32_t R, const uint8_t* ids,
                                     const int64_t* id_offs, int32_t n_ids, const uint8_t* letters, const int64_t* letter_offs, int32_t k,
                                     float digitisation, float range, float offset, const int16_t* dac, int32_t rna,
                                     int32_t with_header, int32_t threads, uint8_t* out, int64_t capacity) {
    const double dig_d = digitisation, range_d = range, offset_d = offset;
    const EventWidths w = event_widths(dig_d, range_d, offset_d);
    if (R < 0 || n_ids < 0 || te < 1 || k < 1 || threads < 1 || capacity < 0 || !w.ok) return S2S_ERR_ARG;
    if (!out) return S2S_ERR_ARG;
    int64_t head = 0;
    char header[sizeof kEventsHeader + 16];
    if (with_header) head = std::snprintf(header, sizeof header, "%s%s\n", kEventsHeader, dac ? "\tsamples" : "");
    if (R == 0) {
        if (n_ids != 0 || head > capacity) return S2S_ERR_ARG;
        std::memcpy(out, header, head);
        return head;
    }
    if (!seg || !sum || !sumsq || !read_first || !read_kmers || !read_offs || !id_offs || !letters || !letter_offs || (n_ids > 0 && !ids))
        return S2S_ERR_ARG;
    std::vector<int32_t> id_of(R);
    std::vector<int64_t> slot(R + 1), size(R, 0);
    int32_t used = 0;
    slot[0] = head;
    for (int r = 0; r < R; ++r) {
        const int64_t chunks = (int64_t)read_first[r + 1] - read_first[r], n = read_offs[r + 1] - read_offs[r];
        if (chunks < 0 || n < 0 || read_kmers[r] < 0 || read_kmers[r] > chunks * te) return S2S_ERR_ARG;
        id_of[r] = -1;
        slot[r + 1] = slot[r];
        if (n == 0) continue;                                    // no samples: no record, no rows
        if (used >= n_ids || id_offs[used + 1] < id_offs[used] || read_kmers[r] < 1) return S2S_ERR_ARG;
        if (letter_offs[r + 1] - letter_offs[r] < read_kmers[r] + k - 1) return S2S_ERR_ARG;
        id_of[r] = used++;
        const int idx_digits = dec_digits((uint64_t)std::max(read_kmers[r], n));
        slot[r + 1] += event_rows_bound(std::min(read_kmers[r], n), id_offs[used] - id_offs[used - 1], k, idx_digits, w, dac ? n : 0);
    }
    if (used != n_ids || slot[R] > capacity) return S2S_ERR_ARG;
    std::atomic<int> failed{0};
    {
        std::lock_guard<std::mutex> guard(g_pool_mutex);
        if (!g_pool || g_pool->size() < threads) { delete g_pool; g_pool = new Pool(threads); }
        g_pool->run(R, [&](int r, int) {
            if (id_of[r] < 0) return;
            const int64_t b0 = read_first[r], chunks = (int64_t)read_first[r + 1] - b0;
            const int64_t K = read_kmers[r], len = read_offs[r + 1] - read_offs[r];
            int64_t total = 0;
            for (int64_t e = b0 * (te + 1); e < (b0 + chunks) * (te + 1); ++e) total += seg[e];
            if (total != len) { failed = 1; return; }            // seg and the export's offsets describe different signals
            uint8_t* p = out + slot[r];
            uint8_t* const end = out + slot[r + 1];
            const uint8_t* id = ids + id_offs[id_of[r]];
            const int64_t id_len = id_offs[id_of[r] + 1] - id_offs[id_of[r]];
            const uint8_t* seq = letters + letter_offs[r];
            const int16_t* stored = dac ? dac + read_offs[r] : nullptr;
            // a number of at most `width` characters and the separator behind it, or the read fails and nothing is written
            // (cannot happen within event_widths' bound)
            auto put_f = [&](const char* fmt, double v, int width, char sep) {
                char tmp[400];
                const int n = std::snprintf(tmp, sizeof tmp, fmt, v);
                if (n < 0 || n > width || end - p < n + 1) { failed = 1; return false; }
                std::memcpy(p, tmp, n); p += n; *p++ = (uint8_t)sep;
                return true;
            };
            int64_t cur = 0;                                      // forward cursor in the read's stored samples
            for (int64_t c = 0; c < chunks && !failed; ++c) {
                const int64_t row = (b0 + c) * (te + 1);
                for (int j = 0; j <= te; ++j) {
                    const int64_t n = seg[row + j], pos = c * te + j, s0 = cur;
                    cur += n;
                    if (!n || j == te || pos >= K) continue;      // an empty k-mer; a tail or a pad k-mer: an insertion
                    const int64_t start = rna ? len - (s0 + n) : s0, stop = start + n;
                    const int64_t S = sum[row + j], Q = sumsq[row + j];
                    const int64_t var = std::max<int64_t>(n * Q - S * S, 0);
                    const double mean = ((double)S / (double)n + offset_d) * range_d / dig_d;
                    const double stdv = std::sqrt((double)var) / (double)n * range_d / dig_d;
                    if (end - p < id_len + k + dec_digits((uint64_t)pos) + dec_digits((uint64_t)start) + dec_digits((uint64_t)stop) + 5) {
                        failed = 1; return;                       // (the slot's bound holds every row: not reached)
                    }
                    std::memcpy(p, id, id_len); p += id_len; *p++ = '\t';
                    p = put_u64(p, pos); *p++ = '\t';
                    std::memcpy(p, seq + pos, k); p += k; *p++ = '\t';
                    p = put_u64(p, start); *p++ = '\t';
                    p = put_u64(p, stop); *p++ = '\t';
                    if (!put_f("%.4f", mean, w.level, '\t')) return;
                    if (!put_f("%.4f", stdv, w.level, stored ? '\t' : '\n')) return;
                    if (stored)
                        for (int64_t t = start; t < stop; ++t)
                            if (!put_f("%.3f", ((double)stored[t] + offset_d) * range_d / dig_d, w.sample - 1, t + 1 < stop ? ',' : '\n'))
                                return;
                }
            }
            size[r] = p - (out + slot[r]);
        });
    }
    if (failed) return S2S_ERR_ARG;
    std::memcpy(out, header, head);
    int64_t pos = head;
    for (int r = 0; r < R; ++r) {                               // close the gaps, in read order
        if (size[r] && pos != slot[r]) std::memmove(out + pos, out + slot[r], size[r]);
        pos += size[r];
    }
    return pos;
}

// ================================================================================ k-mer table (predict --kmer-table)
// The finished table of s2s_kmer_table_accumulate as text, one row per k-mer that occurred; include/s2s_hip.h states the columns.
// At most 4^10 + 1 rows, once per run: one thread.
namespace {

constexpr char kKmerTableHeader[] = "kmer\tn_occ\tn_events\tn_samples\tlevel_mean\tlevel_stdv\tdwell_mean\tdwell_stdv\n";
constexpr int kKmerFields = 6, kKmerMaxK = 10;

// The width a "%.4f" column can take for ANY int64 counters with this calibration: a level is at most (2^63 + |offset|) *
// |range / digitisation| in magnitude, a dwell at most 2^63.  -> 0 for a calibration that is refused.
inline int kmer_table_width(double dig, double range, double offset) {
    if (!(dig == dig) || !(range == range) || !(offset == offset) || dig == 0.0 || range == 0.0) return 0;
    const double M = std::max((9.3e18 + std::fabs(offset)) * std::fabs(range) / std::fabs(dig) * (1.0 + 1e-9) + 1.0, 9.3e18);
    char tmp[400];
    const int digits = (M < 1e300) ? std::snprintf(tmp, sizeof tmp, "%.0f", M) : 312;
    return 1 + digits + 5;
}

// -> the bytes the rows may take, or -1 for a negative counter (sum alone may be negative)
inline int64_t kmer_table_rows_bound(const int64_t* table, int32_t k, int width) {
    const int64_t rows = ((int64_t)1 << (2 * k)) + 1;
    int64_t used = 0;
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t* f = table + r * kKmerFields;
        if (f[0] < 0 || f[1] < 0 || f[2] < 0 || f[3] < 0 || f[5] < 0) return -1;
        used += f[0] >= 1;
    }
    return used * (k + 3 * 20 + 4 * (int64_t)width + 8);
}

}  // namespace

extern "C" int64_t s2s_kmer_table_format_bound(const int64_t* table, int32_t k, float digitisation, float range, float offset,
                                               int32_t with_header) {
    const int width = kmer_table_width(digitisation, range, offset);
    if (!table || k < 1 || k > kKmerMaxK || !width) return S2S_ERR_ARG;
    const int64_t body = kmer_table_rows_bound(table, k, width);
    if (body < 0) return S2S_ERR_ARG;
    return body + (with_header ? (int64_t)sizeof kKmerTableHeader - 1 : 0);
}

extern "C" int64_t s2s_kmer_table_format(const int64_t* table, int32_t k, float digitisation, float range, float offset,
                                         int32_t with_header, uint8_t* out, int64_t capacity) {
    const double dig_d = digitisation, range_d = range, offset_d = offset;
    const int64_t bound = s2s_kmer_table_format_bound(table, k, digitisation, range, offset, with_header);
    if (bound < 0 || !out || capacity < bound) return S2S_ERR_ARG;
    typedef __int128 i128;
    uint8_t* p = out;
    if (with_header) { std::memcpy(p, kKmerTableHeader, sizeof kKmerTableHeader - 1); p += sizeof kKmerTableHeader - 1; }
    const int64_t rows = ((int64_t)1 << (2 * k)) + 1;
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t* f = table + r * kKmerFields;
        if (f[0] < 1) continue;
        for (int i = 0; i < k; ++i) *p++ = (r == rows - 1) ? 'N' : "ACGT"[(r >> (2 * (k - 1 - i))) & 3];
        *p++ = '\t';
        p = put_u64(p, (uint64_t)f[0]); *p++ = '\t';
        p = put_u64(p, (uint64_t)f[1]); *p++ = '\t';
        p = put_u64(p, (uint64_t)f[2]); *p++ = '\t';
        const i128 e = f[1], n = f[2], nn = f[3], S = f[4], Q = f[5];
        if (e == 0) {
            std::memcpy(p, "nan\tnan\tnan\tnan\n", 16); p += 16;
            continue;
        }
        const i128 lv = n * Q - S * S, dv = e * nn - n * n;
        const double v[4] = {((double)S / (double)n + offset_d) * range_d / dig_d,
                             std::sqrt((double)(lv > 0 ? lv : (i128)0)) / (double)n * range_d / dig_d,
                             (double)n / (double)e,
                             std::sqrt((double)(dv > 0 ? dv : (i128)0)) / (double)e};
        for (int i = 0; i < 4; ++i) {
            char tmp[400];
            const int len = std::snprintf(tmp, sizeof tmp, "%.4f", v[i]);
            if (len < 0 || out + capacity - p < len + 1) return S2S_ERR_ARG;      // (the bound holds every number: not reached)
            std::memcpy(p, tmp, len); p += len; *p++ = i < 3 ? '\t' : '\n';
        }
    }
    return p - out;
}

// ================================================================================ k-mer model (predict --kmer-model)
// The fixed-point statistics of one event as a plain entry (the kernel calls the same inline function), and the finished table of
// s2s_kmer_model_accumulate as a nanopolish-style model file; include/s2s_hip.h states both.  One thread, once per run.
extern "C" int s2s_event_fixed(int32_t n, int32_t S, int64_t Q, int64_t* M, int64_t* D) {
    if (n < 1 || n > 1024 || !M || !D) return S2S_ERR_ARG;
    s2s_event_fixed_point(n, S, Q, *M, *D);
    return S2S_OK;
}

namespace {

constexpr char kKmerModelColumns[] = "kmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\tn_events\n";
constexpr int kModelFields = 5;

inline int64_t kmer_model_header_bytes(int32_t k) {
    char tmp[64];
    return std::snprintf(tmp, sizeof tmp, "#k\t%d\n#alphabet\tnucleotide\n", k) + (int64_t)sizeof kKmerModelColumns - 1;
}

// -> the bytes the rows may take, or -1 for a negative counter (sum_m alone may be negative); the row 4^k is never printed
inline int64_t kmer_model_rows_bound(const int64_t* table, int32_t k, int width) {
    const int64_t rows = ((int64_t)1 << (2 * k)) + 1;
    int64_t used = 0;
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t* f = table + r * kModelFields;
        if (f[0] < 0 || f[2] < 0 || f[3] < 0 || f[4] < 0) return -1;
        used += (f[0] >= 1 && r < rows - 1);
    }
    return used * (k + 20 + 4 * (int64_t)width + 6);
}

}  // namespace

extern "C" int64_t s2s_kmer_model_format_bound(const int64_t* table, int32_t k, float digitisation, float range, float offset,
                                               int32_t with_header) {
    const int width = kmer_table_width(digitisation, range, offset);       // (a level is at most 2^63 / 256 counts: the table's width holds)
    if (!table || k < 1 || k > kKmerMaxK || !width) return S2S_ERR_ARG;
    const int64_t body = kmer_model_rows_bound(table, k, width);
    if (body < 0) return S2S_ERR_ARG;
    return body + (with_header ? kmer_model_header_bytes(k) : 0);
}

extern "C" int64_t s2s_kmer_model_format(const int64_t* table, int32_t k, float digitisation, float range, float offset,
                                         int32_t with_header, uint8_t* out, int64_t capacity) {
    const double dig_d = digitisation, range_d = range, offset_d = offset;
    const int64_t bound = s2s_kmer_model_format_bound(table, k, digitisation, range, offset, with_header);
    if (bound < 0 || !out || capacity < bound) return S2S_ERR_ARG;
    typedef __int128 i128;
    uint8_t* p = out;
    if (with_header) {
        p += std::snprintf(reinterpret_cast<char*>(p), 64, "#k\t%d\n#alphabet\tnucleotide\n", k);
        std::memcpy(p, kKmerModelColumns, sizeof kKmerModelColumns - 1); p += sizeof kKmerModelColumns - 1;
    }
    const int64_t rows = (int64_t)1 << (2 * k);                 // (without the extra row)
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t* f = table + r * kModelFields;
        if (f[0] < 1) continue;
        for (int i = 0; i < k; ++i) *p++ = "ACGT"[(r >> (2 * (k - 1 - i))) & 3];
        *p++ = '\t';
        const i128 e = f[0], A = f[1], A2 = f[2], Bs = f[3], B2 = f[4];
        const i128 lv = e * A2 - A * A, sv = e * B2 - Bs * Bs;
        const double den = 256.0 * (double)e;
        const double v[4] = {((double)A / den + offset_d) * range_d / dig_d,
                             std::sqrt((double)(lv > 0 ? lv : (i128)0)) / den * range_d / dig_d,
                             (double)Bs / den * range_d / dig_d,
                             std::sqrt((double)(sv > 0 ? sv : (i128)0)) / den * range_d / dig_d};
        for (int i = 0; i < 4; ++i) {
            char tmp[400];
            const int len = std::snprintf(tmp, sizeof tmp, "%.4f", v[i]);
            if (len < 0 || out + capacity - p < len + 22) return S2S_ERR_ARG;     // (the bound holds every number: not reached)
            std::memcpy(p, tmp, len); p += len; *p++ = '\t';
        }
        p = put_u64(p, (uint64_t)f[0]); *p++ = '\n';
    }
    return p - out;
}

// ================================================================================ read-sampler replay
// The reference samples reads one after the other from Python's global `random` (Mersenne Twister): per attempt a start
// position (random.randint), a strand (random.choice, DNA only), and per N of an accepted read a replacement base; the read
// length comes from scipy with a per-(read, retry) seed (utils.py:311-331, 415-479).  Every draw consumes a data-dependent
// number of generator words, so a rank that owns reads lo..hi of a sharded run can only find the generator state of read lo by
// replaying the draws of reads 0..lo-1 -- 4.3 us per read in the interpreter, a few tens of ns here.  Nothing is built: the
// function walks the draws, returns the accepted reads' lengths and leaves the generator where the next read starts.
namespace {

struct Mt19937 {                      // CPython's _randommodule.c generator: state = random.getstate()[1] (624 words + index)
    uint32_t* mt;
    uint32_t idx;
    uint32_t next() {
        if (idx >= 624) {
            int kk;
            for (kk = 0; kk < 624 - 397; ++kk) {
                const uint32_t y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
                mt[kk] = mt[kk + 397] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            for (; kk < 623; ++kk) {
                const uint32_t y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
                mt[kk] = mt[kk + (397 - 624)] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            const uint32_t y = (mt[623] & 0x80000000u) | (mt[0] & 0x7fffffffu);
            mt[623] = mt[396] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            idx = 0;
        }
        uint32_t y = mt[idx++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        return y;
    }
    // random._randbelow_with_getrandbits(n), 0 < n < 2^32: k = n.bit_length(); redraw getrandbits(k) until < n
    uint64_t below(uint64_t n) {
        int k = 0;
        for (uint64_t t = n; t; t >>= 1) ++k;
        for (;;) {
            const uint64_t r = (uint64_t)(next() >> (32 - k));
            if (r < n) return r;
        }
    }
};

inline uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// draw_expon_dis(mean = r, seed): scipy's expon.rvs(loc, scale, size = 1, random_state = seed) builds np.random.RandomState(seed)
// (init_genrand) and takes loc + scale * -log(1 - random_sample()); then int(x * r / 7106), clipped to [1, total_len]
// (reference utils.py:325-331).  Only the generator's first two outputs are needed: state words 0-2, 397, 398.
struct MtWords { uint32_t w0, w1, w2, w397, w398; };

#pragma clang fp contract(off)
int64_t expon_from_words(const MtWords& w, double r, int64_t total_len) {
    auto twist = [](uint32_t a, uint32_t b, uint32_t c) {
        const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
        return c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    };
    const uint32_t a = mt_temper(twist(w.w0, w.w1, w.w397)) >> 5, b = mt_temper(twist(w.w1, w.w2, w.w398)) >> 6;
    const double u = ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
    const double e = -std::log(1.0 - u);
    const double loc = 213.98910256668592, scale = 6972.5319847131141, fitted_mean = 7106.0;
    double v = scale * e;
    v = loc + v;
    v = v * r;
    v = v / fitted_mean;
    int64_t n = (int64_t)v;                                  // numpy .astype(int): truncation
    if (n < 1) n = 1;
    if (n > total_len) n = total_len;
    return n;
}

int64_t expon_length(uint32_t seed, double r, int64_t total_len) {
    uint32_t x = seed;
    MtWords w{seed, 0, 0, 0, 0};
    for (uint32_t i = 1; i < 399; ++i) {
        x = 1812433253u * (x ^ (x >> 30)) + i;
        if (i == 1) w.w1 = x; else if (i == 2) w.w2 = x; else if (i == 397) w.w397 = x; else if (i == 398) w.w398 = x;
    }
    return expon_from_words(w, r, total_len);
}

// ---- the other two length laws (reference utils.py:311-322): scipy's gamma.rvs / beta.rvs on a fresh np.random.RandomState(seed)
// are numpy's LEGACY samplers (legacy-distributions.c): standard_gamma by Marsaglia-Tsang on legacy_gauss (the polar method, which
// keeps its second variate for the next call -- also across the two gammas of a beta) and 53-bit doubles of MT19937.  They consume
// a variable number of generator outputs, so the whole state is seeded (623 multiplies, ~1 us per (read, try)).
struct NpLegacy {
    uint32_t mt[624];
    int pos = 624;
    bool has_gauss = false;
    double gauss = 0.0;
    explicit NpLegacy(uint32_t seed) {
        mt[0] = seed;
        for (uint32_t i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i;
    }
    uint32_t next() {
        if (pos >= 624) {
            Mt19937 g{mt, 624};
            (void)g.next();                                       // regenerates the block (and tempers word 0, which we redo below)
            pos = 0;
        }
        return mt_temper(mt[pos++]);
    }
    double dbl() {
        const uint32_t a = next() >> 5, b = next() >> 6;
        return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
    }
    double normal() {
        if (has_gauss) { has_gauss = false; const double t = gauss; gauss = 0.0; return t; }
        double f, x1, x2, r2;
        do {
            x1 = 2.0 * dbl() - 1.0;
            x2 = 2.0 * dbl() - 1.0;
            r2 = x1 * x1 + x2 * x2;
        } while (r2 >= 1.0 || r2 == 0.0);
        f = std::sqrt(-2.0 * std::log(r2) / r2);
        gauss = f * x1;
        has_gauss = true;
        return f * x2;
    }
    double std_gamma(double shape) {                              // shape > 1 (both laws)
        const double b = shape - 1.0 / 3.0, c = 1.0 / std::sqrt(9.0 * b);
        for (;;) {
            double X, V;
            do {
                X = normal();
                V = 1.0 + c * X;
            } while (V <= 0.0);
            V = V * V * V;
            const double U = dbl();
            if (U < 1.0 - 0.0331 * (X * X) * (X * X)) return b * V;
            if (std::log(U) < 0.5 * X * X + b * (1.0 - V + std::log(V))) return b * V;
        }
    }
};

// law 0: expon (above); 1: gamma.rvs(6.3693711, loc = 0.53834893) * r / 4.39; 2: beta.rvs(1.778, 7.892, loc = 316.758,
// scale = 34191.257) * r / 6615 -- scipy returns vals * scale + loc; then int(), clipped to [1, total_len]
int64_t law_length(int32_t law, uint32_t seed, double r, int64_t total_len) {
    if (law == 0) return expon_length(seed, r, total_len);
    NpLegacy g(seed);
    double v, fitted;
    if (law == 1) {
        v = g.std_gamma(6.3693711);
        v = v * 1.0 + 0.53834893;
        fitted = 4.39;
    } else {
        const double ga = g.std_gamma(1.778), gb = g.std_gamma(7.892);
        v = ga / (ga + gb);
        v = v * 34191.257;
        v = v + 316.758;
        fitted = 6615.0;
    }
    v = v * r;
    v = v / fitted;
    int64_t n = (int64_t)v;
    if (n < 1) n = 1;
    if (n > total_len) n = total_len;
    return n;
}

// The seeding recurrence is a serial chain of 398 multiplies per seed (0.5 us): eight seeds at a time fill the lanes of one AVX2
// register (the first tries of eight consecutive reads; retries stay scalar).  Same integer arithmetic, lane by lane.
#define S2S_MT_WORDS8_BODY                                                                          \
    uint32_t x[8];                                                                                  \
    for (int l = 0; l < 8; ++l) { x[l] = seeds[l]; out[l].w0 = seeds[l]; }                          \
    for (uint32_t i = 1; i < 399; ++i) {                                                            \
        for (int l = 0; l < 8; ++l) x[l] = 1812433253u * (x[l] ^ (x[l] >> 30)) + i;                 \
        if (i == 1) { for (int l = 0; l < 8; ++l) out[l].w1 = x[l]; }                               \
        else if (i == 2) { for (int l = 0; l < 8; ++l) out[l].w2 = x[l]; }                          \
        else if (i == 397) { for (int l = 0; l < 8; ++l) out[l].w397 = x[l]; }                      \
        else if (i == 398) { for (int l = 0; l < 8; ++l) out[l].w398 = x[l]; }                      \
    }
__attribute__((target("avx2"))) void mt_words8_avx2(const uint32_t* seeds, MtWords* out) { S2S_MT_WORDS8_BODY }
void mt_words8_plain(const uint32_t* seeds, MtWords* out) { S2S_MT_WORDS8_BODY }
void mt_words8(const uint32_t* seeds, MtWords* out) {
    static const bool avx2 = __builtin_cpu_supports("avx2") && !std::getenv("S2S_NO_AVX2");      // (the variable: tests of the plain path)
    if (avx2) mt_words8_avx2(seeds, out); else mt_words8_plain(seeds, out);
}

}  // namespace

extern "C" int64_t s2s_sampler_replay_law(uint32_t* mt_state, const int64_t* contig_ends, int32_t n_contigs,
                                          const int64_t* const* n_pos, const int64_t* n_pos_count, int64_t num_seqs, int64_t first_read_i, int64_t r,
                                          uint64_t seed, int64_t total_len, int32_t is_dna, int32_t min_read_len, int32_t max_retries,
                                          int64_t stop_after, int32_t law, int32_t* out_lengths, int64_t* out_next_read_i) {
    if (!mt_state || !contig_ends || n_contigs < 1 || num_seqs < 0 || first_read_i < 0 || r <= 0 || max_retries < 1 || !out_next_read_i ||
        law < 0 || law > 2)
        return S2S_ERR_ARG;
    const int64_t genome = contig_ends[n_contigs - 1];
    if (genome < 1 || genome >= (1ll << 31) || mt_state[624] > 624) return S2S_ERR_ARG;
    if (seed + (uint64_t)num_seqs * (uint64_t)(max_retries + 1) >= (1ull << 32)) return S2S_ERR_ARG;   // (the scipy seed must not wrap)
    Mt19937 g{mt_state, mt_state[624]};
    int64_t accepted = 0, read_i = first_read_i;
    int64_t first_try[8], first_base = -1;                    // lengths of the first tries of reads first_base .. first_base + 7
    for (; read_i < num_seqs && (stop_after < 0 || accepted < stop_after); ++read_i) {
        if (law == 0 && (first_base < 0 || read_i >= first_base + 8)) {
            uint32_t seeds[8];
            MtWords w[8];
            for (int l = 0; l < 8; ++l) seeds[l] = (uint32_t)(seed + (uint64_t)(read_i + l) * (uint64_t)(max_retries + 1));
            mt_words8(seeds, w);
            for (int l = 0; l < 8; ++l) first_try[l] = expon_from_words(w[l], (double)r, total_len);
            first_base = read_i;
        }
        for (int retry = 0; retry < max_retries; ++retry) {
            const int64_t pos = (int64_t)g.below((uint64_t)genome);                 // random.randint(0, total_genome_len - 1)
            const int64_t* ce = std::upper_bound(contig_ends, contig_ends + n_contigs, pos);   // bisect_right
            const int where = (int)(ce - contig_ends);
            const int64_t start = where ? contig_ends[where - 1] : 0, offset = pos - start, clen = contig_ends[where] - start;
            const int64_t length = (retry == 0 && law == 0) ? first_try[read_i - first_base]
                                              : law_length(law, (uint32_t)(seed + (uint64_t)read_i * (uint64_t)(max_retries + 1) + (uint64_t)retry),
                                                           (double)r, total_len);
            const int64_t got = std::min(length, clen - offset);                     // genome[offset : offset + length]
            if (is_dna) (void)g.below(2);                                           // random.choice("+-")
            if (is_dna && got != length) continue;                                  // read_check: end-of-contig rejection
            if (got < min_read_len) continue;
            int64_t n_count = 0;
            if (n_pos && n_pos[where]) {                                            // read.count("N"): sorted N positions of the contig
                const int64_t* p0 = n_pos[where], *p1 = p0 + n_pos_count[where];
                n_count = std::lower_bound(p0, p1, offset + got) - std::lower_bound(p0, p1, offset);
                if ((double)n_count > 0.1 * (double)length) continue;
            }
            for (int64_t i = 0; i < n_count; ++i) (void)g.below(4);                 // fill_unknown_bases: one choice("ACGT") per N
            if (out_lengths) out_lengths[accepted] = (int32_t)got;
            ++accepted;
            break;
        }
    }
    mt_state[624] = g.idx;
    *out_next_read_i = read_i;
    return accepted;
}

extern "C" int64_t s2s_sampler_replay(uint32_t* mt_state, const int64_t* contig_ends, int32_t n_contigs,
                                      const int64_t* const* n_pos, const int64_t* n_pos_count, int64_t num_seqs, int64_t first_read_i, int64_t r,
                                      uint64_t seed, int64_t total_len, int32_t is_dna, int32_t min_read_len, int32_t max_retries,
                                      int64_t stop_after, int32_t* out_lengths, int64_t* out_next_read_i) {
    return s2s_sampler_replay_law(mt_state, contig_ends, n_contigs, n_pos, n_pos_count, num_seqs, first_read_i, r, seed, total_len, is_dna,
                                  min_read_len, max_retries, stop_after, 0, out_lengths, out_next_read_i);
}

// One read length of law 0 / 1 / 2 (expon / gamma / beta) for a scipy seed: the test hook of the three laws.
extern "C" int64_t s2s_length_law(int32_t law, uint32_t seed, double r, int64_t total_len) {
    if (law < 0 || law > 2 || !(r > 0) || total_len < 1) return S2S_ERR_ARG;
    return law_length(law, seed, r, total_len);
}

// ---- FASTA text -> cleaned sequences (replaces the line loop of utils.read_fasta + process_genome, reference utils.py:290-308,
// 594-597, for plain FASTA files): every rank of a sharded run parses the whole reference before its first kernel.
namespace {
inline bool fa_blank(uint8_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }
// Bytes the text-mode line loop treats differently from this byte-level parser: anything >= 0x80 (the loop decodes UTF-8 -- a name
// keeps its characters, an invalid sequence raises -- and U+0085 / U+00A0 are blanks for str.split) and 0x1c-0x1f (blanks for
// str.split / str.strip as well).  A file that holds one is left to the line loop.
inline bool odd_bytes(const uint8_t* data, int64_t n) {
    unsigned any = 0;
    for (int64_t k = 0; k < n; ++k) any |= (unsigned)(data[k] >= 0x80) | (unsigned)((uint8_t)(data[k] - 0x1c) < 4);
    return any != 0;
}
}  // namespace

// Number of records ('>' in column 0, as pysam / the line loop of utils.read_fasta take it); -2 when the first non-empty line
// starts with '@' (FASTQ: s2s_fastq_clean); -3 when a line holds a carriage return that is not part of its line end (a line
// break of its own under Python's universal newlines: left to the caller's line loop; found by tools/fuzz_host.py).
extern "C" int64_t s2s_fasta_count(const uint8_t* data, int64_t n) {
    if (!data || n < 0) return S2S_ERR_ARG;
    int64_t i = 0, recs = 0;
    bool first = true;
    if (odd_bytes(data, n)) return -3;
    const bool has_cr = n > 0 && std::memchr(data, '\r', (size_t)n) != nullptr;      // (Unix files: one pass, no per-line check)
    while (i < n) {
        const uint8_t* nl = static_cast<const uint8_t*>(std::memchr(data + i, '\n', (size_t)(n - i)));
        int64_t end = nl ? nl - data : n;
        const int64_t next = end + 1;
        if (end > i && data[end - 1] == '\r') --end;                                 // "\r\n" is ONE line end; a second CR in front of it is a line of its own
        if (has_cr && end > i && std::memchr(data + i, '\r', (size_t)(end - i))) return -3;   // a lone CR inside (or at the end of) a line
        if (end > i) {
            if (first && data[i] == '@') return -2;
            first = false;
            recs += data[i] == '>';
        }
        i = next;
    }
    return recs;
}

// out receives the records' sequences back to back: line ends removed, every line stripped of blanks at both ends (as the line
// loop does), optionally upper-cased with everything but ACGT mapped to N (map_acgtn = 1: process_genome).  seq_offs[r],
// seq_offs[r+1] delimit record r in out; name_span[2r], name_span[2r+1] delimit its name (the header's first token) in data.
// Lines before the first header are ignored.  Returns the number of records (<= max_records, else -1).
extern "C" int64_t s2s_fasta_clean(const uint8_t* data, int64_t n, int32_t map_acgtn, uint8_t* out, int64_t* seq_offs,
                                   int64_t* name_span, int64_t max_records) {
    if (!data || n < 0 || !out || !seq_offs || !name_span || max_records < 0) return S2S_ERR_ARG;
    uint8_t tab[256];
    for (int c = 0; c < 256; ++c) {
        uint8_t u = (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : (uint8_t)c;
        tab[c] = map_acgtn ? ((u == 'A' || u == 'C' || u == 'G' || u == 'T') ? u : (uint8_t)'N') : (uint8_t)c;
    }
    int64_t i = 0, recs = 0, o = 0;
    while (i < n) {
        const uint8_t* nl = static_cast<const uint8_t*>(std::memchr(data + i, '\n', (size_t)(n - i)));
        int64_t end = nl ? nl - data : n;
        const int64_t next = end + 1;
        while (end > i && data[end - 1] == '\r') --end;
        if (end > i) {
            if (data[i] == '>') {
                if (recs == max_records) return -1;
                seq_offs[recs] = o;
                int64_t s = i + 1;
                while (s < end && fa_blank(data[s])) ++s;
                int64_t e = s;
                while (e < end && !fa_blank(data[e])) ++e;
                name_span[2 * recs] = s;
                name_span[2 * recs + 1] = e;
                ++recs;
            } else if (recs > 0) {
                int64_t a2 = i, b2 = end;
                while (a2 < b2 && fa_blank(data[a2])) ++a2;
                while (b2 > a2 && fa_blank(data[b2 - 1])) --b2;
                if (map_acgtn) {
                    for (int64_t k = a2; k < b2; ++k) out[o + (k - a2)] = tab[data[k]];
                } else {
                    std::memcpy(out + o, data + a2, (size_t)(b2 - a2));
                }
                o += b2 - a2;
            }
        }
        i = next;
    }
    seq_offs[recs] = o;
    return recs;
}

// FASTQ text (four-line records, as the line loop of utils.read_fasta takes them: blank lines are skipped in front of a header only,
// the sequence line is kept as it stands minus its line end, the third line must start with '+', the fourth is skipped) -> the
// sequences back to back in `out` (>= n bytes; map_acgtn as in s2s_fasta_clean), seq_offs [records + 1], name_span [2 * records]
// (the header's first token inside data).  Returns the number of records; -1 when there are more than max_records; -2 for
// anything the line loop must judge itself (no '@' where a header should be, a missing '+', a truncated last record, a lone
// carriage return inside a line -- a line break for Python's universal newlines).  max_records = 0 with out == NULL only counts.
extern "C" int64_t s2s_fastq_clean(const uint8_t* data, int64_t n, int32_t map_acgtn, uint8_t* out, int64_t* seq_offs,
                                   int64_t* name_span, int64_t max_records) {
    if (!data || n < 0 || max_records < 0) return S2S_ERR_ARG;
    const bool count_only = out == nullptr;
    if (!count_only && (!seq_offs || !name_span)) return S2S_ERR_ARG;
    uint8_t tab[256];
    for (int c = 0; c < 256; ++c) {
        uint8_t u = (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : (uint8_t)c;
        tab[c] = map_acgtn ? ((u == 'A' || u == 'C' || u == 'G' || u == 'T') ? u : (uint8_t)'N') : (uint8_t)c;
    }
    int64_t i = 0, recs = 0, o = 0;
    bool bad = false;
    if (odd_bytes(data, n)) return -2;
    auto line = [&](int64_t& b, int64_t& e) {                // next line [b, e) without its line end; false at the end of the data
        if (i >= n) return false;
        const uint8_t* nl = static_cast<const uint8_t*>(std::memchr(data + i, '\n', (size_t)(n - i)));
        e = nl ? nl - data : n;
        b = i;
        i = e + 1;
        if (e > b && data[e - 1] == '\r') --e;                 // one CR belongs to the line end; any other is a line break of its own
        if (e > b && std::memchr(data + b, '\r', (size_t)(e - b))) bad = true;
        return true;
    };
    int64_t b, e;
    while (line(b, e)) {
        if (bad) return -2;
        if (e == b) continue;
        if (data[b] != '@') return -2;
        int64_t s = b + 1;
        while (s < e && fa_blank(data[s])) ++s;
        int64_t t = s;
        while (t < e && !fa_blank(data[t])) ++t;
        int64_t sb, se, pb, pe, qb, qe;
        if (!line(sb, se) || !line(pb, pe) || !line(qb, qe) || bad) return -2;
        if (pe == pb || data[pb] != '+') return -2;
        if (!count_only) {
            if (recs == max_records) return -1;
            seq_offs[recs] = o;
            name_span[2 * recs] = s;
            name_span[2 * recs + 1] = t;
            if (map_acgtn) {
                for (int64_t k = sb; k < se; ++k) out[o + (k - sb)] = tab[data[k]];
            } else {
                std::memcpy(out + o, data + sb, (size_t)(se - sb));
            }
            o += se - sb;
        }
        ++recs;
    }
    if (!count_only) seq_offs[recs] = o;
    return recs;
}

// ---- rank-shard merge (`predict --gpus N`, `merge-shards`): the reference writes ONE file (inference.py:65-79), a sharded run
// writes one per rank, and joining them must not cost more than the ranks' parallel phase did.  Both helpers work on file
// descriptors; nothing passes through the interpreter or (copy_file_range) through user space.
#include <cerrno>
#include <climits>
#include <fcntl.h>
#include <map>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/vfs.h>
#include <unistd.h>

namespace {

int64_t copy_one(int src, int64_t src_off, int dst, int64_t dst_off, int64_t len, std::vector<uint8_t>& bounce, bool& in_kernel) {
    while (len > 0) {
        if (in_kernel) {
            off_t so = (off_t)src_off, d_o = (off_t)dst_off;
            const ssize_t r = copy_file_range(src, &so, dst, &d_o, (size_t)std::min<int64_t>(len, 1 << 30), 0);
            if (r > 0) { src_off += r; dst_off += r; len -= r; continue; }
            if (r == 0) return -EIO;                                 // source shorter than the caller said
            if (errno == EINTR) continue;
            if (errno != EXDEV && errno != ENOSYS && errno != EINVAL && errno != EOPNOTSUPP && errno != EPERM) return -errno;
            in_kernel = false;                                      // another file system / an old kernel: through a bounce buffer
        }
        if (bounce.empty()) bounce.resize(8 << 20);
        const ssize_t r = pread(src, bounce.data(), (size_t)std::min<int64_t>(len, (int64_t)bounce.size()), (off_t)src_off);
        if (r == 0) return -EIO;
        if (r < 0) { if (errno == EINTR) continue; return -errno; }
        for (ssize_t done = 0; done < r;) {
            const ssize_t w = pwrite(dst, bounce.data() + done, (size_t)(r - done), (off_t)(dst_off + done));
            if (w < 0) { if (errno == EINTR) continue; return -errno; }
            done += w;
        }
        src_off += r; dst_off += r; len -= r;
    }
    return 0;
}

}  // namespace

// Two engines.
//  * descriptors (engine 0): copy_file_range, in the kernel.  One destination file has ONE fast writer this way: buffered writes
//    take its inode lock, so 2-8 threads into the SAME file are slower than one (3.2-4.1 against 6.5 GB/s on the MI355X box's tmpfs,
//    profiles/r05/fs_write_probe_shm.txt), and what a lone writer spends its time on is allocating the destination's pages.
//  * preallocate + mapped fill (engine 1, tmpfs destinations): posix_fallocate() the destination ranges first -- allocation WITHOUT
//    data runs at 18.6 GB/s there -- then `threads` threads each map-populate a 16-MiB piece of the destination (MADV_POPULATE_WRITE:
//    one call instead of a trap per page) and pread() the source straight into it: the kernel copies from the source's page cache
//    into pages that already exist -- no inode lock, no allocation.  8.0 GB/s against 5.7 GB/s for engine 0 on the same box
//    (profiles/r05/merge_bench_shm.txt; memcpy from a source mapping instead of pread: 6.1; without the populate call: 6.7; with the
//    next range's fallocate running beside the copy: 4.0 -- it slows the faults down).  The space is reserved before the first store,
//    so a full file system is an error code (the fallocate fails, engine 0 takes over and reports ENOSPC), never a SIGBUS.  On a
//    disk file system's page cache the same engine LOSES (3.7-4.5 against 7-10 GB/s: fallocate is a block allocation there), so
//    engine 1 is only taken for tmpfs.  (Round 5's first mapped engine, commit 1b15c95, stored into pages that did NOT exist yet and
//    lost everywhere: the page allocation under the faults was the bound.)
namespace {
struct Span { int64_t lo = INT64_MAX, hi = 0; uint8_t* base = nullptr; size_t bytes = 0; };      // the hull of a file's ranges, and its mapping

bool map_spans(std::map<int, Span>& spans) {
    for (auto& kv : spans) {
        Span& sp = kv.second;
        sp.lo &= ~(int64_t)4095;                                     // (mmap wants a page-aligned file offset)
        sp.bytes = (size_t)(sp.hi - sp.lo);
        void* m = mmap(nullptr, sp.bytes, PROT_READ | PROT_WRITE, MAP_SHARED, kv.first, (off_t)sp.lo);
        if (m == MAP_FAILED) { sp.base = nullptr; return false; }
        sp.base = static_cast<uint8_t*>(m);
    }
    return true;
}
void unmap_spans(std::map<int, Span>& spans) {
    for (auto& kv : spans)
        if (kv.second.base) munmap(kv.second.base, kv.second.bytes);
}
}  // namespace

extern "C" int64_t s2s_copy_ranges(int32_t n, const int32_t* src_fd, const int64_t* src_off, const int32_t* dst_fd,
                                   const int64_t* dst_off, const int64_t* len, int32_t threads, int32_t engine) {
    if (n < 0 || threads < 1 || engine < 0 || engine > 2 || (n > 0 && (!src_fd || !src_off || !dst_fd || !dst_off || !len))) return S2S_ERR_ARG;
    // pieces of <= 16 MiB, so that one long range does not leave the other threads idle
    struct Piece { int src, dst; int64_t so, d_o, len; };
    std::vector<Piece> pieces;
    const int64_t cut = 16ll << 20;
    int64_t total = 0;
    std::map<int, Span> dsts;
    std::map<int, int64_t> src_end;
    for (int i = 0; i < n; ++i) {
        if (len[i] < 0 || src_off[i] < 0 || dst_off[i] < 0) return S2S_ERR_ARG;
        if (len[i] == 0) continue;
        for (int64_t o = 0; o < len[i]; o += cut)
            pieces.push_back({src_fd[i], dst_fd[i], src_off[i] + o, dst_off[i] + o, std::min(cut, len[i] - o)});
        total += len[i];
        src_end[src_fd[i]] = std::max(src_end[src_fd[i]], src_off[i] + len[i]);
        Span& b = dsts[dst_fd[i]];
        b.lo = std::min(b.lo, dst_off[i]); b.hi = std::max(b.hi, dst_off[i] + len[i]);
    }
    if (pieces.empty()) return 0;
    bool mapped = engine >= 1;
    if (mapped)
        for (auto& kv : dsts) {
            struct stat st;
            struct statfs fs;
            if (src_end.count(kv.first) || fstat(kv.first, &st) != 0 || !S_ISREG(st.st_mode)) { mapped = false; break; }   // (a file copied onto itself: descriptors)
            if (engine == 1 && (fstatfs(kv.first, &fs) != 0 || fs.f_type != 0x01021994)) { mapped = false; break; }       // TMPFS_MAGIC (engine 2: any file system, A/B)
            if (posix_fallocate(kv.first, (off_t)kv.second.lo, (off_t)(kv.second.hi - kv.second.lo)) != 0) { mapped = false; break; }
        }
    if (mapped) {
        mapped = map_spans(dsts);
        if (!mapped) unmap_spans(dsts);
    }
    // every piece's destination mapping is looked up HERE, on one thread: the workers only read the vector (std::map::operator[] is
    // a non-const member, and concurrent calls of it are a data race on paper even when every key exists)
    std::vector<const Span*> span_of(pieces.size(), nullptr);
    if (mapped)
        for (size_t i = 0; i < pieces.size(); ++i) span_of[i] = &dsts.find(pieces[i].dst)->second;
    std::atomic<size_t> next{0};
    std::atomic<int64_t> err{0};
    auto work = [&] {
        std::vector<uint8_t> bounce;
        bool in_kernel = true;
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= pieces.size() || err.load()) return;
            const Piece& p = pieces[i];
            if (mapped) {
                const Span& b = *span_of[i];
                uint8_t* to = b.base + (p.d_o - b.lo);
#ifdef MADV_POPULATE_WRITE
                const uintptr_t lo = (uintptr_t)to & ~(uintptr_t)4095, hi = ((uintptr_t)to + (uintptr_t)p.len + 4095) & ~(uintptr_t)4095;
                (void)madvise((void*)lo, hi - lo, MADV_POPULATE_WRITE);        // (Linux 5.14+; refused elsewhere: plain faults)
#endif
                int64_t done = 0;
                while (done < p.len) {                                       // a source shorter than its range ends the call with -EIO, no fault
                    const ssize_t r = pread(p.src, to + done, (size_t)(p.len - done), (off_t)(p.so + done));
                    if (r <= 0) { if (r < 0 && errno == EINTR) continue; err = r < 0 ? -errno : -EIO; break; }
                    done += r;
                }
                continue;
            }
            const int64_t r = copy_one(p.src, p.so, p.dst, p.d_o, p.len, bounce, in_kernel);
            if (r < 0) err = r;
        }
    };
    const int workers = (int)std::min<size_t>((size_t)(mapped ? threads : 1), std::max<size_t>(pieces.size(), 1));   // (descriptors: one writer)
    std::vector<std::thread> pool;
    for (int w = 1; w < workers; ++w) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    if (mapped) unmap_spans(dsts);
    return err.load() < 0 ? err.load() : total;
}

extern "C" int64_t s2s_blow5_scan(int32_t fd, int64_t begin, int64_t end) {
    if (fd < 0 || begin < 0 || end < begin) return S2S_ERR_ARG;
    int64_t pos = begin, n = 0;
    while (pos < end) {
        uint64_t size;
        if (end - pos < 8 || pread(fd, &size, 8, (off_t)pos) != 8) return -2;
        if (size > (uint64_t)(end - pos - 8)) return -2;                // a record runs past the end-of-file marker: truncated shard
        pos += 8 + (int64_t)size;
        ++n;
    }
    return n;
}

// The same walk over a file that is still being written (the live join tails the rank files while the ranks run): complete records
// only -- a size prefix or a body that reaches past `limit` (the file's size at the moment of the call) ends the walk without an
// error -- and at most max_records of them.  *out_end = the byte offset behind the last complete record.
extern "C" int64_t s2s_blow5_scan_upto(int32_t fd, int64_t begin, int64_t limit, int64_t max_records, int64_t* out_end) {
    if (fd < 0 || begin < 0 || !out_end) return S2S_ERR_ARG;
    int64_t pos = begin, n = 0;
    while (n < max_records && limit - pos >= 8) {
        uint64_t size;
        if (pread(fd, &size, 8, (off_t)pos) != 8) break;
        if (size > (uint64_t)(limit - pos - 8)) break;                 // body not (yet) whole: the writer is in the middle of it, or this is the end marker
        pos += 8 + (int64_t)size;
        ++n;
    }
    *out_end = pos;
    return n;
}


// ================================================================================ compare: median / MAD, normalise, banded DTW on the host
// The plain-C++ twins of the three kernels of s2s_dtw.h (include/s2s_hip.h states the definitions): `compare --cpu`, and what the
// kernels must equal bit for bit.  Records / pairs are dealt out over host threads; nothing is shared between them.
#include "s2s_dtw.h"

namespace {

template <class F>
void dtw_for_each(int32_t n, int32_t threads, F fn) {
    std::atomic<int32_t> next{0};
    auto work = [&]() {
        for (int32_t i; (i = next.fetch_add(1)) < n;) fn(i);
    };
    const int extra = std::min<int32_t>(threads, n) - 1;
    std::vector<std::thread> pool;
    for (int t = 0; t < extra; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
}

bool dtw_offsets_ok(const int64_t* offs, int32_t n) {
    for (int32_t i = 0; i < n; ++i) {
        const int64_t len = offs[i + 1] - offs[i];
        if (len < 0 || len > S2S_DTW_MAX_SAMPLES) return false;
    }
    return true;
}

inline int64_t dtw_floor_div(int64_t a, int64_t b) {       // b > 0
    int64_t q = a / b;
    return a - q * b < 0 ? q - 1 : q;
}

// Row sweep: row i holds the columns jlo(i) .. jhi(i) = ceil((i m - T) / n) .. floor((i m + T) / n) clipped to the matrix; two rolling
// rows indexed by j - jlo of their own row; a predecessor outside its row's range is +infinity.
int64_t dtw_pair(const int16_t* a, int64_t n, const int16_t* b, int64_t m, int64_t R) {
    if (n <= 0 || m <= 0) return S2S_DTW_COST_EMPTY;
    const int64_t T = R * std::max(n, m);
    const int64_t width = std::min<int64_t>(m, 2 * (T / n) + 3);
    std::vector<int64_t> rows(2 * (size_t)width);
    int64_t* prev = rows.data();
    int64_t* cur = prev + width;
    int64_t plo = 0, phi = -1;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t jlo = std::max<int64_t>(0, -dtw_floor_div(T - i * m, n)), jhi = std::min(m - 1, dtw_floor_div(i * m + T, n));
        for (int64_t j = jlo; j <= jhi; ++j) {
            int64_t best = (i == 0 && j == 0) ? 0 : S2S_DTW_UNREACHED;
            if (j >= plo && j <= phi) best = std::min(best, prev[j - plo]);                  // (i - 1, j)
            if (j - 1 >= plo && j - 1 <= phi) best = std::min(best, prev[j - 1 - plo]);      // (i - 1, j - 1)
            if (j - 1 >= jlo) best = std::min(best, cur[j - 1 - jlo]);                       // (i, j - 1)
            const int64_t c = std::abs((int64_t)a[i] - (int64_t)b[j]);
            cur[j - jlo] = best >= S2S_DTW_UNREACHED ? S2S_DTW_UNREACHED : best + c;
        }
        std::swap(prev, cur);
        plo = jlo; phi = jhi;
    }
    return (m - 1 >= plo && m - 1 <= phi) ? prev[m - 1 - plo] : S2S_DTW_UNREACHED;
}

// dtw_pair with the path: the same sweep, the predecessors taken in the order of the tie rule (diagonal, up, left; '<' keeps the
// earlier one), 2 bits per cell in `stride` 64-bit words per row (cell j of row i at bit pair j - jlo(i)), then the walk back from
// (n - 1, m - 1).  The k-th op of the walk is ops_end[-1 - k]; -> the cost, *steps = the ops written.
int64_t dtw_pair_path(const int16_t* a, int64_t n, const int16_t* b, int64_t m, int64_t R, uint8_t* ops_end, int64_t* steps) {
    *steps = 0;
    if (n <= 0 || m <= 0) return S2S_DTW_COST_EMPTY;
    const int64_t T = R * std::max(n, m);
    const int64_t width = std::min<int64_t>(m, 2 * (T / n) + 3), stride = (width + 31) / 32;
    std::vector<int64_t> rows(2 * (size_t)width);
    std::vector<uint64_t> dec((size_t)n * (size_t)stride, 0);
    int64_t* prev = rows.data();
    int64_t* cur = prev + width;
    int64_t plo = 0, phi = -1;
    auto row_lo = [&](int64_t i) { return std::max<int64_t>(0, -dtw_floor_div(T - i * m, n)); };
    for (int64_t i = 0; i < n; ++i) {
        const int64_t jlo = row_lo(i), jhi = std::min(m - 1, dtw_floor_div(i * m + T, n));
        uint64_t* drow = dec.data() + (size_t)i * (size_t)stride;
        for (int64_t j = jlo; j <= jhi; ++j) {
            int64_t best = S2S_DTW_UNREACHED;
            uint64_t code = S2S_DTW_OP_NONE;
            if (j - 1 >= plo && j - 1 <= phi && prev[j - 1 - plo] < best) { best = prev[j - 1 - plo]; code = S2S_DTW_OP_M; }
            if (j >= plo && j <= phi && prev[j - plo] < best) { best = prev[j - plo]; code = S2S_DTW_OP_A; }
            if (j - 1 >= jlo && cur[j - 1 - jlo] < best) { best = cur[j - 1 - jlo]; code = S2S_DTW_OP_B; }
            if (i == 0 && j == 0) best = 0;
            const int64_t c = std::abs((int64_t)a[i] - (int64_t)b[j]);
            cur[j - jlo] = best >= S2S_DTW_UNREACHED ? S2S_DTW_UNREACHED : best + c;
            drow[(j - jlo) >> 5] |= code << (2 * ((j - jlo) & 31));
        }
        std::swap(prev, cur);
        plo = jlo; phi = jhi;
    }
    const int64_t cost = (m - 1 >= plo && m - 1 <= phi) ? prev[m - 1 - plo] : S2S_DTW_UNREACHED;
    if (cost >= S2S_DTW_UNREACHED) return cost;
    int64_t i = n - 1, j = m - 1, k = 0;
    while ((i | j) != 0 && k < n + m - 2) {
        const int64_t x = j - row_lo(i);
        if (x < 0 || x >= width) break;
        const unsigned code = (unsigned)(dec[(size_t)i * (size_t)stride + (size_t)(x >> 5)] >> (2 * (x & 31))) & 3u;
        const int64_t di = code != S2S_DTW_OP_B, dj = code != S2S_DTW_OP_A;
        if (code == S2S_DTW_OP_NONE || i < di || j < dj) break;
        ops_end[-1 - k] = (uint8_t)code;
        ++k;
        i -= di;
        j -= dj;
    }
    *steps = (i | j) == 0 ? k : 0;
    return cost;
}

}  // namespace

extern "C" int s2s_signal_median_mad_host(const int16_t* samples, const int64_t* offs, int32_t R, int32_t* med, int32_t* mad, int32_t threads) {
    if (R < 0 || threads < 1 || !offs || (R > 0 && (!samples || !med || !mad)) || !dtw_offsets_ok(offs, R)) return S2S_ERR_ARG;
    dtw_for_each(R, threads, [&](int32_t r) {
        const int64_t n = offs[r + 1] - offs[r];
        if (n == 0) { med[r] = 0; mad[r] = 0; return; }
        const int16_t* p = samples + offs[r];
        const int64_t k = (n - 1) / 2;
        std::vector<int32_t> v(p, p + n);
        std::nth_element(v.begin(), v.begin() + k, v.end());
        const int32_t md = v[k];
        for (int64_t i = 0; i < n; ++i) v[i] = std::abs((int32_t)p[i] - md);
        std::nth_element(v.begin(), v.begin() + k, v.end());
        med[r] = md; mad[r] = v[k];
    });
    return S2S_OK;
}

extern "C" int s2s_signal_normalise_host(const int16_t* samples, const int64_t* offs, int32_t R, const int32_t* med, const int32_t* mad,
                                         int32_t scale, int16_t* out, int32_t threads) {
    if (R < 0 || threads < 1 || !offs || scale < 1 || scale > S2S_DTW_MAX_SCALE || (R > 0 && (!samples || !med || !mad || !out)) ||
        !dtw_offsets_ok(offs, R))
        return S2S_ERR_ARG;
    dtw_for_each(R, threads, [&](int32_t r) {
        for (int64_t i = offs[r]; i < offs[r + 1]; ++i) out[i] = s2s_dtw_normalise_one(samples[i], med[r], mad[r], scale);
    });
    return S2S_OK;
}

extern "C" int s2s_dtw_banded_host(const int16_t* a, const int64_t* a_offs, const int16_t* b, const int64_t* b_offs, int32_t P, int32_t band,
                                   int64_t* cost, int32_t threads) {
    if (P < 0 || threads < 1 || band < 1 || band > S2S_DTW_MAX_BAND || !a_offs || !b_offs || (P > 0 && (!a || !b || !cost)) ||
        !dtw_offsets_ok(a_offs, P) || !dtw_offsets_ok(b_offs, P))
        return S2S_ERR_ARG;
    dtw_for_each(P, threads, [&](int32_t p) {
        cost[p] = dtw_pair(a + a_offs[p], a_offs[p + 1] - a_offs[p], b + b_offs[p], b_offs[p + 1] - b_offs[p], band);
    });
    return S2S_OK;
}

extern "C" int s2s_dtw_path_host(const int16_t* a, const int64_t* a_offs, const int16_t* b, const int64_t* b_offs, int32_t P, int32_t band,
                                 int64_t* cost, uint8_t* ops, const int64_t* path_offs, int64_t* steps, int32_t threads) {
    if (P < 0 || threads < 1 || band < 1 || band > S2S_DTW_MAX_BAND || !a_offs || !b_offs || !path_offs ||
        (P > 0 && (!a || !b || !cost || !ops || !steps)) || !dtw_offsets_ok(a_offs, P) || !dtw_offsets_ok(b_offs, P))
        return S2S_ERR_ARG;
    for (int32_t p = 0; p < P; ++p) {               // every pair's slot holds its longest path
        const int64_t n = a_offs[p + 1] - a_offs[p], m = b_offs[p + 1] - b_offs[p];
        if (path_offs[p] < 0 || path_offs[p + 1] - path_offs[p] < (n > 0 && m > 0 ? n + m - 2 : 0)) return S2S_ERR_ARG;
    }
    dtw_for_each(P, threads, [&](int32_t p) {
        cost[p] = dtw_pair_path(a + a_offs[p], a_offs[p + 1] - a_offs[p], b + b_offs[p], b_offs[p + 1] - b_offs[p], band,
                                ops + path_offs[p + 1], &steps[p]);
    });
    return S2S_OK;
}

// ================================================================================ compare --open-ends: subsequence DTW on the host
// The definition of include/s2s_hip.h (next to s2s_sdtw) as a row sweep with two rolling rows of (E, S); reverse reads q and t back
// to front through the index, no copy.  What the kernel of s2s_sdtw.h must equal bit for bit.
namespace {

void sdtw_one(const int16_t* q, int64_t L, const int16_t* t, int64_t H, bool rev, int64_t* cost, int64_t* start, int64_t* end) {
    *start = 0;
    *end = 0;
    if (L <= 0 || H <= 0) { *cost = S2S_DTW_COST_EMPTY; return; }
    struct Cell { int32_t e, s; };
    std::vector<Cell> rows(2 * (size_t)H);
    Cell* prev = rows.data();
    Cell* cur = prev + H;
    auto qa = [&](int64_t i) { return (int32_t)(rev ? q[L - 1 - i] : q[i]); };
    auto ta = [&](int64_t j) { return (int32_t)(rev ? t[H - 1 - j] : t[j]); };
    for (int64_t j = 0; j < H; ++j) cur[j] = Cell{std::abs(qa(0) - ta(j)), (int32_t)j};
    for (int64_t i = 1; i < L; ++i) {
        std::swap(prev, cur);
        const int32_t x = qa(i);
        cur[0] = Cell{prev[0].e + std::abs(x - ta(0)), prev[0].s};
        for (int64_t j = 1; j < H; ++j) {
            Cell b = prev[j - 1];                                   // (i - 1, j - 1), then (i - 1, j), then (i, j - 1): '<' keeps the earlier
            if (prev[j].e < b.e) b = prev[j];
            if (cur[j - 1].e < b.e) b = cur[j - 1];
            cur[j] = Cell{b.e + std::abs(x - ta(j)), b.s};
        }
    }
    int64_t js = 0;
    for (int64_t j = 1; j < H; ++j)
        if (cur[j].e < cur[js].e) js = j;
    *cost = cur[js].e;
    *start = rev ? H - (js + 1) : cur[js].s;
    *end = rev ? H - cur[js].s : js + 1;
}

}  // namespace

extern "C" int s2s_sdtw_host(const int16_t* q, const int64_t* q_begin, const int64_t* q_len, const int16_t* t, const int64_t* t_begin,
                             const int64_t* t_len, const uint8_t* reverse, int32_t P, int64_t* cost, int64_t* start, int64_t* end,
                             int32_t threads) {
    if (P < 0 || threads < 1 || (P > 0 && (!q || !q_begin || !q_len || !t || !t_begin || !t_len || !reverse || !cost || !start || !end)))
        return S2S_ERR_ARG;
    for (int32_t p = 0; p < P; ++p)
        if (q_begin[p] < 0 || t_begin[p] < 0 || q_len[p] < 0 || t_len[p] < 0 || q_len[p] > S2S_SDTW_MAX_QUERY ||
            t_len[p] > S2S_DTW_MAX_SAMPLES)
            return S2S_ERR_ARG;
    dtw_for_each(P, threads, [&](int32_t p) {
        sdtw_one(q + q_begin[p], q_len[p], t + t_begin[p], t_len[p], reverse[p] != 0, &cost[p], &start[p], &end[p]);
    });
    return S2S_OK;
}

// ================================================================================ resquiggle: signal against k-mer levels on the host
// The definition of include/s2s_hip.h (next to s2s_resquiggle) as a row sweep: row i holds the columns jlo(i) .. jhi(i) =
// max(0, ceil(i K / n) - R) .. min(K - 1, floor(i K / n) + R); two rolling rows indexed by j - jlo of their own row; 2 bits per
// in-band cell; then the walk back.  What the kernels of s2s_resquiggle.h must equal bit for bit.
#include "s2s_resquiggle.h"

namespace {

int64_t rsq_one(const int16_t* q, int64_t n, const int16_t* l, int64_t K, int64_t R, int64_t skip, int64_t unknown, int32_t* start,
                int32_t* len) {
    for (int64_t j = 0; j < K; ++j) { start[j] = -1; len[j] = 0; }
    if (n <= 0 || K <= 0) return S2S_DTW_COST_EMPTY;
    if (K > 2 * n) return S2S_RSQ_UNREACHED;
    const int64_t width = std::min<int64_t>(K, 2 * R + 1), stride = (width + 31) / 32;
    std::vector<int64_t> rows(2 * (size_t)width, S2S_DTW_UNREACHED);
    std::vector<uint64_t> dec((size_t)n * (size_t)stride, 0);
    int64_t* prev = rows.data();
    int64_t* cur = prev + width;
    int64_t plo = 0, phi = -1;
    auto row_lo = [&](int64_t i) { return std::max<int64_t>(0, (i * K + n - 1) / n - R); };
    auto at = [&](int64_t j) { return j >= plo && j <= phi ? prev[j - plo] : S2S_DTW_UNREACHED; };
    for (int64_t i = 0; i < n; ++i) {
        const int64_t jlo = row_lo(i), jhi = std::min(K - 1, i * K / n + R);
        uint64_t* drow = dec.data() + (size_t)i * (size_t)stride;
        for (int64_t j = jlo; j <= jhi; ++j) {
            int64_t best = S2S_DTW_UNREACHED;
            uint64_t code = S2S_RSQ_NONE;
            if (at(j - 1) < best) { best = at(j - 1); code = S2S_RSQ_ADV; }
            if (at(j) < best) { best = at(j); code = S2S_RSQ_STAY; }
            const int64_t t2 = at(j - 2) >= S2S_DTW_UNREACHED ? S2S_DTW_UNREACHED : at(j - 2) + skip;
            if (t2 < best) { best = t2; code = S2S_RSQ_SKIP; }
            if (i == 0) { best = j == 0 ? 0 : S2S_DTW_UNREACHED; code = S2S_RSQ_NONE; }
            const int64_t c = l[j] == S2S_RSQ_UNKNOWN ? unknown : std::abs((int64_t)q[i] - (int64_t)l[j]);
            cur[j - jlo] = best >= S2S_DTW_UNREACHED ? S2S_DTW_UNREACHED : best + c;
            drow[(j - jlo) >> 5] |= (best >= S2S_DTW_UNREACHED ? (uint64_t)S2S_RSQ_NONE : code) << (2 * ((j - jlo) & 31));
        }
        std::swap(prev, cur);
        plo = jlo; phi = jhi;
    }
    const int64_t cost = at(K - 1);
    if (cost >= S2S_DTW_UNREACHED) return S2S_RSQ_UNREACHED;
    int64_t i = n - 1, j = K - 1, run = 0;
    bool arrived = false;
    for (;;) {
        ++run;
        if (i == 0) {
            arrived = j == 0;
            if (arrived) { start[0] = 0; len[0] = (int32_t)run; }
            break;
        }
        const int64_t x = j - row_lo(i);
        if (x < 0 || x >= width) break;
        const unsigned code = (unsigned)(dec[(size_t)i * (size_t)stride + (size_t)(x >> 5)] >> (2 * (x & 31))) & 3u;
        if (code == S2S_RSQ_NONE) break;
        if (code != S2S_RSQ_STAY) {
            const int64_t dj = code == S2S_RSQ_ADV ? 1 : 2;
            if (j < dj) break;
            start[j] = (int32_t)i; len[j] = (int32_t)run;
            run = 0;
            j -= dj;
        }
        --i;
    }
    if (!arrived)                                   // (never: a reached corner has a path)
        for (int64_t t = 0; t < K; ++t) { start[t] = -1; len[t] = 0; }
    return cost;
}

}  // namespace

extern "C" int s2s_resquiggle_host(const int16_t* q, const int64_t* q_offs, const int16_t* l, const int64_t* l_offs, int32_t P, int32_t band,
                                   int32_t skip_penalty, int32_t unknown_cost, int64_t* cost, int32_t* ev_start, int32_t* ev_len,
                                   int32_t threads) {
    if (P < 0 || threads < 1 || band < 1 || band > S2S_DTW_MAX_BAND || skip_penalty < 0 || skip_penalty > S2S_RSQ_MAX_SKIP_PENALTY ||
        unknown_cost < 0 || unknown_cost > S2S_RSQ_MAX_UNKNOWN_COST || !q_offs || !l_offs ||
        (P > 0 && (!q || !l || !cost || !ev_start || !ev_len)) || !dtw_offsets_ok(q_offs, P) || !dtw_offsets_ok(l_offs, P) ||
        (P > 0 && l_offs[0] < 0))
        return S2S_ERR_ARG;
    dtw_for_each(P, threads, [&](int32_t p) {
        cost[p] = rsq_one(q + q_offs[p], q_offs[p + 1] - q_offs[p], l + l_offs[p], l_offs[p + 1] - l_offs[p], band, skip_penalty,
                          unknown_cost, ev_start + l_offs[p], ev_len + l_offs[p]);
    });
    return S2S_OK;
}

extern "C" int s2s_event_sums_host(const int16_t* samples, const int64_t* s_offs, const int32_t* ev_start, const int32_t* ev_len,
                                   const int64_t* l_offs, int32_t P, int64_t* S, int64_t* Q, int32_t threads) {
    if (P < 0 || threads < 1 || !s_offs || !l_offs || (P > 0 && (!samples || !ev_start || !ev_len || !S || !Q))) return S2S_ERR_ARG;
    for (int32_t p = 0; p < P; ++p)
        if (s_offs[p + 1] < s_offs[p] || l_offs[p + 1] < l_offs[p] || l_offs[0] < 0) return S2S_ERR_ARG;
    dtw_for_each(P, threads, [&](int32_t p) {
        const int64_t n = s_offs[p + 1] - s_offs[p];
        for (int64_t j = l_offs[p]; j < l_offs[p + 1]; ++j) {
            const int64_t b = ev_start[j], len = ev_len[j];
            int64_t s1 = 0, s2 = 0;
            if (b >= 0 && len > 0 && b + len <= n)
                for (int64_t t = 0; t < len; ++t) {
                    const int64_t x = samples[s_offs[p] + b + t];
                    s1 += x;
                    s2 += x * x;
                }
            S[j] = s1; Q[j] = s2;
        }
    });
    return S2S_OK;
}

// ================================================================================ segment: event detection on the host
// The definition of include/s2s_hip.h (next to s2s_segment) record by record: the window sums from prefix sums, the two detectors'
// scores over [0, n], the peaks, the merge rule, the events.  What the kernels of s2s_segment.h must equal bit for bit.
#include "s2s_segment.h"

namespace {

// score_w(i) for i = 0 .. n into sc [n + 1]; ps / pq [n + 1]: prefix sums of x and x^2
void seg_scores(const std::vector<int64_t>& ps, const std::vector<int64_t>& pq, int64_t n, int32_t w, std::vector<int64_t>& sc) {
    std::fill(sc.begin(), sc.begin() + n + 1, 0);
    for (int64_t i = w; i + w <= n; ++i)
        sc[i] = s2s_seg_score((int32_t)(ps[i] - ps[i - w]), (int32_t)(ps[i + w] - ps[i]), pq[i + w] - pq[i - w], w);
}

// peaks of one detector into pk [n + 1]
void seg_peaks(const std::vector<int64_t>& sc, int64_t n, int32_t w, int64_t thr, std::vector<uint8_t>& pk) {
    std::fill(pk.begin(), pk.begin() + n + 1, 0);
    for (int64_t i = 0; i <= n; ++i) {
        const int64_t v = sc[i];
        if (v < thr) continue;
        bool p = true;
        for (int64_t j = std::max<int64_t>(0, i - w); j < i && p; ++j) p = v > sc[j];
        for (int64_t j = i + 1; j <= std::min(n, i + w) && p; ++j) p = v >= sc[j];
        pk[i] = p;
    }
}

struct SegWork {
    std::vector<int64_t> ps, pq, sc;
    std::vector<uint8_t> pk_s, pk_l;
    std::vector<int32_t> bounds;
};

// -> the record's boundaries (ascending) in wk.bounds
void seg_one(const int16_t* x, int64_t n, int32_t w_s, int32_t w_l, int64_t t_s, int64_t t_l, SegWork& wk) {
    wk.bounds.clear();
    if (n < 2 * w_s) return;                         // no position has a score
    const size_t m = (size_t)n + 1;
    if (wk.ps.size() < m) { wk.ps.resize(m); wk.pq.resize(m); wk.sc.resize(m); wk.pk_s.resize(m); wk.pk_l.resize(m); }
    wk.ps[0] = wk.pq[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t v = x[i];
        wk.ps[i + 1] = wk.ps[i] + v;
        wk.pq[i + 1] = wk.pq[i] + v * v;
    }
    seg_scores(wk.ps, wk.pq, n, w_s, wk.sc);
    seg_peaks(wk.sc, n, w_s, t_s, wk.pk_s);
    seg_scores(wk.ps, wk.pq, n, w_l, wk.sc);
    seg_peaks(wk.sc, n, w_l, t_l, wk.pk_l);
    for (int64_t i = 0; i <= n; ++i) {
        bool b = wk.pk_s[i];
        if (!b && wk.pk_l[i]) {
            b = true;
            for (int64_t j = std::max<int64_t>(0, i - w_s); j <= std::min(n, i + w_s) && b; ++j) b = !wk.pk_s[j];
        }
        if (b) wk.bounds.push_back((int32_t)i);
    }
}

}  // namespace

extern "C" int64_t s2s_segment_capacity(int64_t n, int32_t w_short) {
    if (n < 0 || w_short < 1 || w_short > S2S_SEG_MAX_WINDOW) return S2S_ERR_ARG;
    return n == 0 ? 0 : std::max<int64_t>(1, n / w_short);
}

extern "C" int s2s_segment_host(const int16_t* samples, const int64_t* offs, int32_t R, int64_t total, int32_t w_short, int32_t w_long,
                                int64_t thr_short, int64_t thr_long, const int64_t* ev_offs, int32_t* ev_start, int32_t* ev_len,
                                int32_t* n_events, int32_t threads) {
    if (R < 0 || total < 0 || threads < 1 || !s2s_seg_params_ok(w_short, w_long, thr_short, thr_long) || !offs || !ev_offs ||
        (R > 0 && (!n_events || (total > 0 && (!samples || !ev_start || !ev_len)))) || !dtw_offsets_ok(offs, R) ||
        (R > 0 && (offs[0] < 0 || offs[R] > total)))
        return S2S_ERR_ARG;
    std::atomic<int32_t> next{0}, small{0};
    auto work = [&]() {
        SegWork wk;
        for (int32_t r; (r = next.fetch_add(1)) < R;) {
            const int64_t n = offs[r + 1] - offs[r];
            if (n == 0) { n_events[r] = 0; continue; }
            seg_one(samples + offs[r], n, w_short, w_long, thr_short, thr_long, wk);
            const int64_t cnt = (int64_t)wk.bounds.size() + 1, eo = ev_offs[r], cap = ev_offs[r + 1] - eo;
            if (eo < 0 || cnt > cap) { n_events[r] = (int32_t)-cnt; small = 1; continue; }
            int64_t at = 0;
            for (int64_t k = 0; k < cnt; ++k) {
                const int64_t end = k + 1 < cnt ? wk.bounds[k] : n;
                ev_start[eo + k] = (int32_t)at;
                ev_len[eo + k] = (int32_t)(end - at);
                at = end;
            }
            n_events[r] = (int32_t)cnt;
        }
    };
    const int extra = std::min<int32_t>(threads, R) - 1;
    std::vector<std::thread> pool;
    for (int t = 0; t < extra; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    return small ? S2S_ERR_ARG : S2S_OK;
}

namespace {

constexpr char kSegmentHeader[] = "read_name\tevent_index\tstart_idx\tend_idx\tevent_level_mean\tevent_stdv\n";
constexpr int64_t kSegmentBlock = 4096;             // rows of one unit of formatting work

// bytes one row of record r may take, or -1 for a calibration that is refused
inline int64_t segment_row_bound(int64_t id_len, const double* cal) {
    if (!std::isfinite(cal[0]) || !std::isfinite(cal[1]) || !std::isfinite(cal[2])) return -1;
    const EventWidths w = event_widths(cal[0], cal[2], cal[1]);
    if (!w.ok) return -1;
    return id_len + 3 * 10 + 2 * (int64_t)w.level + 6;     // three int32 numbers, two levels, five tabs and the line end
}

}  // namespace

extern "C" int64_t s2s_segment_format_bound(const int32_t* n_events, int32_t R, const int64_t* id_offs, const double* cal,
                                            int32_t with_header) {
    if (R < 0 || (R > 0 && (!n_events || !id_offs || !cal))) return S2S_ERR_ARG;
    int64_t total = with_header ? (int64_t)sizeof kSegmentHeader - 1 : 0;
    for (int32_t r = 0; r < R; ++r) {
        if (id_offs[r + 1] < id_offs[r]) return S2S_ERR_ARG;
        if (n_events[r] <= 0) continue;
        const int64_t row = segment_row_bound(id_offs[r + 1] - id_offs[r], cal + 3 * (int64_t)r);
        if (row < 0) return S2S_ERR_ARG;
        total += row * n_events[r];
    }
    return total;
}

extern "C" int64_t s2s_segment_format(const int32_t* ev_start, const int32_t* ev_len, const int64_t* S, const int64_t* Q,
                                      const int64_t* ev_offs, const int32_t* n_events, int32_t R, const uint8_t* ids, const int64_t* id_offs,
                                      const double* cal, int32_t with_header, int32_t threads, uint8_t* out, int64_t capacity) {
    if (threads < 1 || !out || capacity < 0) return S2S_ERR_ARG;
    const int64_t bound = s2s_segment_format_bound(n_events, R, id_offs, cal, with_header);
    if (bound < 0 || capacity < bound) return S2S_ERR_ARG;
    struct Unit { int32_t r; int64_t k0, k1, at, size; };
    std::vector<Unit> units;
    int64_t head = with_header ? (int64_t)sizeof kSegmentHeader - 1 : 0, at = head;
    std::vector<int64_t> row(R > 0 ? R : 0, 0);
    for (int32_t r = 0; r < R; ++r) {
        if (n_events[r] <= 0) continue;
        if (!ev_start || !ev_len || !S || !Q || !ev_offs || !ids || ev_offs[r] < 0 || ev_offs[r + 1] - ev_offs[r] < n_events[r])
            return S2S_ERR_ARG;
        row[r] = segment_row_bound(id_offs[r + 1] - id_offs[r], cal + 3 * (int64_t)r);
        for (int64_t k0 = 0; k0 < n_events[r]; k0 += kSegmentBlock) {
            const int64_t k1 = std::min<int64_t>(n_events[r], k0 + kSegmentBlock);
            units.push_back(Unit{r, k0, k1, at, 0});
            at += (k1 - k0) * row[r];
        }
    }
    std::atomic<int> failed{0};
    dtw_for_each((int32_t)units.size(), threads, [&](int32_t u) {
        Unit& un = units[u];
        const int32_t r = un.r;
        const double dig = cal[3 * (int64_t)r], offset = cal[3 * (int64_t)r + 1], range = cal[3 * (int64_t)r + 2];
        const uint8_t* id = ids + id_offs[r];
        const int64_t id_len = id_offs[r + 1] - id_offs[r];
        uint8_t* p = out + un.at;
        uint8_t* const end = p + (un.k1 - un.k0) * row[r];
        for (int64_t k = un.k0; k < un.k1; ++k) {
            const int64_t j = ev_offs[r] + k, n = ev_len[j], start = ev_start[j], s = S[j], q = Q[j];
            if (n < 1 || start < 0 || end - p < row[r]) { failed = 1; return; }
            // an event may hold 2^22 samples: n Q passes 2^63, so the difference is formed in 128 bits and rounded once
            const __int128 var = std::max<__int128>((__int128)n * q - (__int128)s * s, 0);
            const double mean = ((double)s / (double)n + offset) * range / dig;
            const double stdv = std::sqrt((double)var) / (double)n * range / dig;
            std::memcpy(p, id, id_len); p += id_len; *p++ = '\t';
            p = put_u64(p, (uint64_t)k); *p++ = '\t';
            p = put_u64(p, (uint64_t)start); *p++ = '\t';
            p = put_u64(p, (uint64_t)(start + n)); *p++ = '\t';
            char tmp[400];
            int c = std::snprintf(tmp, sizeof tmp, "%.4f", mean);
            if (c < 0 || end - p < c + 1) { failed = 1; return; }
            std::memcpy(p, tmp, c); p += c; *p++ = '\t';
            c = std::snprintf(tmp, sizeof tmp, "%.4f", stdv);
            if (c < 0 || end - p < c + 1) { failed = 1; return; }
            std::memcpy(p, tmp, c); p += c; *p++ = '\n';
        }
        un.size = p - (out + un.at);
    });
    if (failed) return S2S_ERR_ARG;
    if (with_header) std::memcpy(out, kSegmentHeader, head);
    int64_t pos = head;
    for (const Unit& un : units) {                                   // close the gaps, in order
        if (un.size && pos != un.at) std::memmove(out + pos, out + un.at, un.size);
        pos += un.size;
    }
    return pos;
}

// ================================================================================ eventalign: event means against k-mer levels on the host
// The definitions of include/s2s_hip.h (next to s2s_event_means and s2s_eventalign) band by band: three rolling bands of W cells, 2
// bits per cell and lk per band, then the walk back.  What the kernels of s2s_eventalign.h must equal bit for bit.
#include "s2s_eventalign.h"

namespace {

struct EvaOut {
    int32_t* first;
    int32_t* end;
    int32_t* kmer;
    int32_t* k_start;
    int32_t* k_len;
    int32_t* k_events;
};

int64_t eva_one(const int16_t* m, int64_t E, const int16_t* l, int64_t K, const int32_t* st, const int32_t* ln, int64_t W, int64_t skip,
                int64_t trim, int64_t unknown, const EvaOut& out) {
    auto clear = [&]() {
        for (int64_t e = 0; e < E; ++e) out.kmer[e] = -1;
        for (int64_t j = 0; j < K; ++j) { out.k_start[j] = -1; out.k_len[j] = 0; out.k_events[j] = 0; }
        *out.first = *out.end = 0;
    };
    clear();
    if (E <= 0 || K <= 0) return S2S_DTW_COST_EMPTY;
    const int64_t bands = E + K - 1;
    std::vector<int64_t> rows(3 * (size_t)W, S2S_DTW_UNREACHED);
    std::vector<uint8_t> dec((size_t)bands * (size_t)(W / 4), 0);
    std::vector<int32_t> lks((size_t)bands);
    int64_t* cur = rows.data();
    int64_t* p1 = cur + W;                          // band b - 1
    int64_t* p2 = p1 + W;                           // band b - 2
    auto at = [&](const int64_t* band, int64_t o) { return o >= 0 && o < W ? band[o] : S2S_DTW_UNREACHED; };
    int64_t lk = -(W / 2), r1 = 0, best = S2S_DTW_UNREACHED, best_e = 0;
    for (int64_t b = 0; b < bands; ++b) {
        int64_t r = 0;
        if (b > 0) {
            const int64_t ll = p1[0], ur = p1[W - 1];
            r = (ll >= S2S_DTW_UNREACHED && ur >= S2S_DTW_UNREACHED) ? (b & 1) : (ll > ur ? 1 : 0);
        }
        lk += r;
        lks[(size_t)b] = (int32_t)lk;
        uint8_t* drow = dec.data() + (size_t)b * (size_t)(W / 4);
        for (int64_t o = 0; o < W; ++o) {
            const int64_t j = lk + o, e = b - j;
            int64_t v = S2S_DTW_UNREACHED;
            unsigned code = S2S_EVA_START;
            if (j >= 0 && j < K && e >= 0 && e < E) {
                const int64_t c = l[j] == S2S_RSQ_UNKNOWN ? unknown : std::abs((int64_t)m[e] - (int64_t)l[j]);
                const int64_t pd = at(p2, o + r + r1 - 1), ps = at(p1, o + r), pk = at(p1, o + r - 1);
                if (j >= 1 && pd < v) { v = pd + c; code = S2S_EVA_DIAG; }
                if (ps < S2S_DTW_UNREACHED && ps + c < v) { v = ps + c; code = S2S_EVA_STAY; }
                if (j >= 1 && pk < S2S_DTW_UNREACHED && pk + skip < v) { v = pk + skip; code = S2S_EVA_SKIP; }
                if (j == 0 && e * trim + c < v) { v = e * trim + c; code = S2S_EVA_START; }
                if (v >= S2S_DTW_UNREACHED) code = S2S_EVA_START;
                if (j == K - 1 && v < S2S_DTW_UNREACHED) {
                    const int64_t f = v + (E - 1 - e) * trim;
                    if (f < best || (f == best && e < best_e)) { best = f; best_e = e; }
                }
            }
            cur[o] = v;
            drow[o >> 2] |= (uint8_t)(code << (2 * (o & 3)));
        }
        r1 = r;
        int64_t* t = p2;
        p2 = p1; p1 = cur; cur = t;
    }
    if (best >= S2S_DTW_UNREACHED) return S2S_RSQ_UNREACHED;
    int64_t e = best_e, j = K - 1, run = 0, hi = 0;
    bool arrived = false;
    for (int64_t step = 0; step < E + K; ++step) {
        const int64_t b = e + j, o = j - lks[(size_t)b];
        if (o < 0 || o >= W) break;
        const unsigned code = (dec[(size_t)b * (size_t)(W / 4) + (size_t)(o >> 2)] >> (2 * (o & 3))) & 3u;
        if (code == S2S_EVA_SKIP) {
            if (run != 0 || j == 0) break;
            --j;
            continue;
        }
        out.kmer[e] = (int32_t)j;
        if (run == 0) hi = e;
        ++run;
        if (code == S2S_EVA_STAY) {
            if (e == 0) break;
            --e;
            continue;
        }
        out.k_start[j] = st[e];
        out.k_len[j] = st[hi] + ln[hi] - st[e];
        out.k_events[j] = (int32_t)run;
        run = 0;
        if (code == S2S_EVA_START) { arrived = j == 0; break; }
        if (e == 0 || j == 0) break;
        --e;
        --j;
    }
    if (!arrived) { clear(); return best; }          // (never: a reached cell has a path)
    *out.first = (int32_t)e;
    *out.end = (int32_t)(best_e + 1);
    return best;
}

}  // namespace

extern "C" int64_t s2s_eventalign_scratch_bytes(int64_t E, int64_t K, int32_t width) {
    if (width < 64 || width > S2S_EVA_MAX_WIDTH || width % 64 != 0) return S2S_ERR_ARG;
    return s2s_eva_bytes(E, K, width);
}

extern "C" int s2s_event_means_host(const int64_t* S, const int32_t* ev_len, const int64_t* ev_offs, const int32_t* n_events, int32_t R,
                                    int64_t capacity, int64_t* m_offs, int16_t* means, int32_t threads) {
    if (R < 0 || capacity < 0 || threads < 1 || !ev_offs || !m_offs || (R > 0 && (!n_events || (capacity > 0 && (!S || !ev_len || !means)))))
        return S2S_ERR_ARG;
    if (R > 0 && ev_offs[0] < 0) return S2S_ERR_ARG;
    for (int32_t r = 0; r < R; ++r)
        if (ev_offs[r + 1] < ev_offs[r]) return S2S_ERR_ARG;
    m_offs[0] = 0;
    for (int32_t r = 0; r < R; ++r) m_offs[r + 1] = m_offs[r] + s2s_eva_count(n_events[r], ev_offs[r], ev_offs[r + 1]);
    if (m_offs[R] > capacity) return S2S_ERR_ARG;
    dtw_for_each(R, threads, [&](int32_t r) {
        const int64_t eo = ev_offs[r], cnt = m_offs[r + 1] - m_offs[r];
        for (int64_t e = 0; e < cnt; ++e) means[m_offs[r] + e] = s2s_eva_mean(S[eo + e], ev_len[eo + e]);
    });
    return S2S_OK;
}

extern "C" int s2s_eventalign_host(const int16_t* m, const int64_t* m_offs, const int16_t* l, const int64_t* l_offs,
                                   const int32_t* ev_start, const int32_t* ev_len, const int64_t* ev_offs, int32_t P, int32_t width,
                                   int32_t skip_penalty, int32_t trim_penalty, int32_t unknown_cost, int64_t* cost, int32_t* first_event,
                                   int32_t* end_event, int32_t* ev_kmer, int32_t* k_start, int32_t* k_len, int32_t* k_events,
                                   int32_t threads) {
    if (P < 0 || threads < 1 || !s2s_eva_params_ok(width, skip_penalty, trim_penalty, unknown_cost) || !m_offs || !l_offs || !ev_offs ||
        (P > 0 && (!m || !l || !ev_start || !ev_len || !cost || !first_event || !end_event || !ev_kmer || !k_start || !k_len || !k_events)) ||
        !dtw_offsets_ok(m_offs, P) || !dtw_offsets_ok(l_offs, P) || (P > 0 && (m_offs[0] < 0 || l_offs[0] < 0)))
        return S2S_ERR_ARG;
    for (int32_t p = 0; p < P; ++p)
        if (ev_offs[p] < 0 || ev_offs[p + 1] - ev_offs[p] < m_offs[p + 1] - m_offs[p]) return S2S_ERR_ARG;
    dtw_for_each(P, threads, [&](int32_t p) {
        const EvaOut out{first_event + p, end_event + p, ev_kmer + m_offs[p], k_start + l_offs[p], k_len + l_offs[p], k_events + l_offs[p]};
        cost[p] = eva_one(m + m_offs[p], m_offs[p + 1] - m_offs[p], l + l_offs[p], l_offs[p + 1] - l_offs[p], ev_start + ev_offs[p],
                          ev_len + ev_offs[p], width, skip_penalty, trim_penalty, unknown_cost, out);
    });
    return S2S_OK;
}

// ================================================================================ preprocess: training chunks on the host
// The definition of include/s2s_hip.h (next to s2s_chunk_pack) read by read: the rows in position order, the pads, the chunks, the
// keep rule.  What the kernels of s2s_chunk.h must equal bit for bit, floats included.
#include "s2s_chunk.h"

extern "C" int64_t s2s_chunk_scratch_bytes(int64_t slots, int32_t P, int64_t chunk_capacity) {
    if (!s2s_chk_counts_ok(P, 0, slots, chunk_capacity)) return S2S_ERR_ARG;
    return s2s_chk_layout(slots, P, chunk_capacity).bytes;
}

extern "C" int s2s_chunk_pack_host(const void* pool, const int64_t* s_offs, int64_t total, int32_t source, const int64_t* l_offs,
                                   int64_t slots, const int32_t* ev_start, const int32_t* ev_len, const int64_t* S, const int64_t* Q,
                                   const double* cal, const float* stdv, const uint8_t* kmers, int32_t P, int32_t k, int32_t te, int32_t ts,
                                   int32_t reverse, int32_t backwards, int64_t chunk_capacity, uint16_t* chunks, int64_t* chunks_lengths,
                                   float* targets, int64_t* targets_lengths, float* stdevs, int32_t* n_rows, int64_t* counters,
                                   int32_t threads) {
    const bool work = P > 0 && slots > 0;
    const bool raw = source == S2S_CHUNK_RAW;
    if (threads < 1 || !s2s_chk_params_ok(source, k, te, ts) || !s2s_chk_counts_ok(P, total, slots, chunk_capacity) || chunk_capacity < P ||
        !s_offs || !l_offs || !counters || (P > 0 && !n_rows) ||
        (work && (!ev_start || !ev_len || !kmers || !chunks || !chunks_lengths || !targets || !targets_lengths || !stdevs ||
                  (total > 0 && !pool) || (raw ? (!S || !Q || !cal) : !stdv))))
        return S2S_ERR_ARG;
    if (P > 0 && (s_offs[0] < 0 || l_offs[0] < 0 || s_offs[P] > total || l_offs[P] != slots)) return S2S_ERR_ARG;
    for (int32_t p = 0; p < P; ++p) {
        if (s_offs[p + 1] < s_offs[p] || l_offs[p + 1] < l_offs[p] || l_offs[p + 1] - l_offs[p] > S2S_DTW_MAX_SAMPLES) return S2S_ERR_ARG;
        if (work && raw && !(std::isfinite(cal[3 * p]) && std::isfinite(cal[3 * p + 1]) && std::isfinite(cal[3 * p + 2]) && cal[3 * p] != 0.0))
            return S2S_ERR_ARG;
    }
    counters[0] = counters[1] = counters[2] = 0;
    for (int32_t p = 0; p < P; ++p) n_rows[p] = 0;
    if (!work) return S2S_OK;

    // the reads' rows, in position order
    std::vector<std::vector<int64_t>> rows((size_t)P);
    std::vector<int64_t> all_n((size_t)P, 0);
    dtw_for_each(P, threads, [&](int32_t p) {
        auto& mine = rows[(size_t)p];
        for (int64_t g = l_offs[p]; g < l_offs[p + 1]; ++g) {
            const int row = s2s_chunk_row(ev_start[g], ev_len[g], s_offs[p], s_offs[p + 1], total, kmers + g * k, k);
            if (row == 1) mine.push_back(g);
            all_n[(size_t)p] += row == 2;
        }
        if (backwards) std::reverse(mine.begin(), mine.end());
        n_rows[p] = (int32_t)mine.size();
    });
    std::vector<int64_t> c_offs((size_t)P + 1, 0);
    for (int32_t p = 0; p < P; ++p) {
        const int64_t n = (int64_t)rows[(size_t)p].size();
        c_offs[(size_t)p + 1] = c_offs[(size_t)p] + (n > 0 ? n / te + 1 : 0);
        counters[2] += all_n[(size_t)p];
    }
    const int64_t formed = c_offs[(size_t)P];
    counters[0] = formed;
    if (formed > chunk_capacity) return S2S_ERR_ARG;
    std::vector<int32_t> read_of((size_t)formed);
    for (int32_t p = 0; p < P; ++p)
        for (int64_t c = c_offs[(size_t)p]; c < c_offs[(size_t)p + 1]; ++c) read_of[(size_t)c] = p;

    // row j of chunk c: its slot, or -1 for a pad; its length
    auto row_of = [&](int64_t c, int32_t j, int64_t& len) {
        const int32_t p = read_of[(size_t)c];
        const auto& mine = rows[(size_t)p];
        const int64_t i = (c - c_offs[(size_t)p]) * te + j;
        if (i >= (int64_t)mine.size()) { len = 1; return (int64_t)-1; }
        len = ev_len[mine[(size_t)i]];
        return mine[(size_t)i];
    };
    std::vector<int64_t> dest((size_t)formed + 1, 0);                       // the kept chunks before chunk c
    dtw_for_each((int32_t)formed, threads, [&](int32_t c) {
        int64_t tl = 0, len;
        for (int32_t j = 0; j < te; ++j) { row_of(c, j, len); tl += len; }
        dest[(size_t)c + 1] = tl <= ts;
    });
    for (int64_t c = 0; c < formed; ++c) dest[(size_t)c + 1] += dest[(size_t)c];
    counters[1] = dest[(size_t)formed];
    dtw_for_each((int32_t)formed, threads, [&](int32_t c) {
        if (dest[(size_t)c + 1] == dest[(size_t)c]) return;
        const int64_t at = dest[(size_t)c];
        const int32_t p = read_of[(size_t)c];
        uint16_t* hot = chunks + at * te * k * 5;
        float* tg = targets + at * ts;
        std::fill(hot, hot + (int64_t)te * k * 5, (uint16_t)0);
        std::fill(tg, tg + ts, 0.0f);
        int64_t t = 0;
        for (int32_t j = 0; j < te; ++j) {
            int64_t len;
            const int64_t g = row_of(c, j, len);
            chunks_lengths[at * te + j] = len;
            float dev = 0.0f;
            for (int32_t q = 0; q < k; ++q) {
                const int32_t col = g < 0 ? 0 : s2s_chunk_column(kmers[g * k + q]);
                if (col >= 0) hot[(j * k + q) * 5 + col] = S2S_CHK_ONE;
            }
            if (g < 0) {
                t += 1;                                                      // (the pad's sample 0.0 is there)
            } else {
                const int64_t first = s_offs[p] + ev_start[g];
                for (int64_t o = 0; o < len; ++o) {
                    const int64_t idx = first + (reverse ? len - 1 - o : o);
                    tg[t++] = raw ? s2s_chunk_pa(static_cast<const int16_t*>(pool)[idx], cal[3 * p], cal[3 * p + 1], cal[3 * p + 2])
                                  : static_cast<const float*>(pool)[idx];
                }
                dev = raw ? s2s_chunk_stdv(len, S[g], Q[g], cal[3 * p], cal[3 * p + 2]) : stdv[g];
            }
            stdevs[at * te + j] = dev;
        }
        targets_lengths[at] = t;
    });
    return S2S_OK;
}

// ================================================================================ the pore model from alignments on the host
// The definition of include/s2s_hip.h (next to s2s_kmer_model_events) record by record and slot by slot, with the slot rule and the
// conversion the kernel calls (s2s_kmer_model_events.h).  What the kernel must equal bit for bit.  One thread: the adds of a run
// meet in a few rows, and the command calls this once per batch behind an alignment that took far longer.
#include "s2s_kmer_model_events.h"

extern "C" int s2s_kmer_model_events_host(const int32_t* codes, const int32_t* ev_len, const int64_t* S, const int64_t* Q,
                                          const int64_t* l_offs, int32_t P, const int64_t* gain, const int64_t* shift, int32_t k,
                                          int64_t* table, int64_t* dropped, int32_t threads) {
    if (k < 1 || k > S2S_KMER_TABLE_MAX_K || P < 0 || threads < 1 ||
        (P > 0 && (!codes || !ev_len || !S || !Q || !l_offs || !gain || !shift || !table || !dropped)))
        return S2S_ERR_ARG;
    for (int32_t p = 0; p < P; ++p)
        if (l_offs[p + 1] < l_offs[p] || l_offs[0] < 0) return S2S_ERR_ARG;
    const int32_t rows = (1 << (2 * k)) + 1;
    for (int32_t p = 0; p < P; ++p) {
        if (gain[p] == 0) continue;
        for (int64_t g = l_offs[p]; g < l_offs[p + 1]; ++g) {
            int64_t Mp = 0, Dp = 0;
            const int what = s2s_kme_slot(ev_len[g], S[g], Q[g], codes[g], rows, gain[p], shift[p], Mp, Dp);
            if (what == S2S_KME_NONE) continue;
            if (what != S2S_KME_EVENT) {
                dropped[what - 1] += 1;             // overlong, out_of_range, bad_code: in the order of `dropped`
                continue;
            }
            int64_t* row = table + (int64_t)codes[g] * S2S_KMER_MODEL_FIELDS;
            row[0] += 1;
            row[1] += Mp;
            row[2] += Mp * Mp;
            row[3] += Dp;
            row[4] += Dp * Dp;
            dropped[3] += 1;
        }
    }
    return S2S_OK;
}
