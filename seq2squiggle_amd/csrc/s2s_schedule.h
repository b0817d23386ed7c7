// How a launch of the predict kernel (s2s_fused_kernel) is dealt out to its persistent workgroups when it is large: a list of
// CLAIMS, taken in order from one counter.  Host and device compute the same list from (n, G, group), so the tests walk it on the
// CPU (s2s_schedule_claim in the C ABI).
//
//   claims 0 .. H-1       whole groups of `group` chunks, H = max(0, (n - G * group) / group)
//   the taper zone        the last Z = n - H * group chunks (G * group <= Z < (G + 1) * group once n >= G * group; all of a
//                         smaller launch): G claims of group / 2, G of group / 4, ..., G of 2, then 2 G + (what is left) of 1,
//                         filled from the small end -- a zone shorter than G * group loses its LARGE claims first
//   claims past the end   count 0
//
// so the sizes never grow from the zone on and the last thing any workgroup starts is one chunk: the launch ends at most about one
// chunk time after its slowest compute unit would have ended under a perfect split.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define S2S_HD __host__ __device__
#else
#define S2S_HD
#endif

// `auto` takes claims from this many groups per workgroup on (a multiple of G * group chunks): below it the taper's extra frontend
// phases cost more than the tail they remove (profiles/r10/README.md)
#define S2S_SCHEDULE_AUTO_GROUPS 8

// claim c of a launch of n chunks on G workgroups -> [start, start + count); count 0 (start n) past the end.  Closed form: the
// loop runs over the log2(group) - 1 claim sizes of the zone, not over c.  (32-bit: a launch is at most 2^20 chunks, and the
// kernel's thread 0 computes this beside a full register file.)
S2S_HD inline void s2s_claim_range(const int n, const int G, const int group, const int c, int* start, int* count) {
    if (c < 0 || n <= 0) { *start = n > 0 ? n : 0; *count = 0; return; }
    const int full = G * group;
    const int H = n > full ? (n - full) / group : 0;
    if (c < H) { *start = c * group; *count = group; return; }
    const int Z = n - H * group;
    int idx = c - H, pos = H * group;
    for (int s = group >> 1; s >= 2; s >>= 1) {
        // the claims below size s hold G * s chunks (2 G singles, G claims each of 2 .. s / 2): size s takes what lies above that
        const int above = Z - G * s;
        int cs = above > 0 ? above / s : 0;
        if (cs > G) cs = G;
        if (idx < cs) { *start = pos + idx * s; *count = s; return; }
        idx -= cs;
        pos += cs * s;
    }
    if (idx < n - pos) { *start = pos + idx; *count = 1; return; }
    *start = n; *count = 0;
}

// what S2S_SCHEDULE = auto decides for a launch of n chunks on G workgroups: claims (true) or the static split
S2S_HD inline bool s2s_auto_takes_claims(const long long n, const int G, const int group) {
    return n >= (long long)S2S_SCHEDULE_AUTO_GROUPS * G * group;
}
