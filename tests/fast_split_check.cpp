// CPU check of the split of k_fast's tile table by level (slam-module_amd/csrc/orb_geom.h: OrbGeom::ftiles_level0, orb_fast_split_auto).  For
// each geometry: every entry of ftile_tab below the level-0 count names level 0, every entry from it on a higher level, the two counts add up
// to ftiles_total, and the automatic rule agrees with a direct count of the workgroups of each part-launch (frames x that part's tiles, each
// more than kFastPruneMinBlocks) for 1, 16, 17, 32 and 256 frames.  Prints "split <w>x<h> <level-0 tiles> <other tiles> <first n_frames that
// splits, 0 = none up to 4096>" per geometry and exits non-zero on the first violation.
#include <cstdio>
#include <vector>

#include "orb_geom.h"

struct Case { int w, h, levels; float scale; };

static bool check(const Case &k) {
    ms_orb_config cfg{};
    cfg.width = k.w; cfg.height = k.h; cfg.levels = k.levels; cfg.scale_factor = k.scale;
    cfg.max_kpts = 1000; cfg.lk_track_level = 0; cfg.fast_threshold = 20; cfg.max_tracks = 0; cfg.max_batch = 256; cfg.min_distance = 0.f;
    OrbGeom R;
    char why[256];
    if (orb_geometry(cfg, R, why, sizeof(why)) != MS_OK) { std::printf("%dx%d: %s\n", k.w, k.h, why); return false; }
    const int total = R.geom.ftiles_total, n0 = R.ftiles_level0;
    if ((size_t)total * 2 != R.ftile_tab.size()) { std::printf("%dx%d: ftiles_total %d, table of %zu dwords\n", k.w, k.h, total, R.ftile_tab.size()); return false; }
    if (n0 < 1 || n0 > total) { std::printf("%dx%d: %d level-0 tiles of %d\n", k.w, k.h, n0, total); return false; }
    int count0 = 0, count1 = 0;                     // a direct count, whatever the order of the table
    for (int t = 0; t < total; ++t) {
        const int l = (int)(R.ftile_tab[2 * (size_t)t] & 15u);
        if (l >= k.levels) { std::printf("%dx%d: entry %d names level %d of %d\n", k.w, k.h, t, l, k.levels); return false; }
        if (t < n0 && l != 0) { std::printf("%dx%d: entry %d (below the level-0 count %d) names level %d\n", k.w, k.h, t, n0, l); return false; }
        if (t >= n0 && l == 0) { std::printf("%dx%d: entry %d (behind the level-0 count %d) names level 0\n", k.w, k.h, t, n0); return false; }
        if (l == 0) ++count0; else ++count1;
    }
    if (count0 != n0 || count0 + count1 != total || n0 + (total - n0) != total) { std::printf("%dx%d: counts %d + %d, table %d / %d\n", k.w, k.h, count0, count1, n0, total); return false; }
    if ((k.levels == 1) != (count1 == 0)) { std::printf("%dx%d: %d levels, %d tiles above level 0\n", k.w, k.h, k.levels, count1); return false; }
    for (int nf : {1, 16, 17, 32, 256}) {
        const bool want = (long long)nf * count0 > kFastPruneMinBlocks && (long long)nf * count1 > kFastPruneMinBlocks;
        const bool got = orb_fast_split_auto(nf, R.ftiles_level0, total);
        if (got != want) { std::printf("%dx%d: %d frames of %d + %d tiles: the rule says %d, the count %d\n", k.w, k.h, nf, count0, count1, (int)got, (int)want); return false; }
    }
    int first = 0;
    for (int nf = 1; nf <= 4096 && !first; ++nf) if (orb_fast_split_auto(nf, R.ftiles_level0, total)) first = nf;
    std::printf("split %dx%d %d %d %d\n", k.w, k.h, count0, count1, first);
    return true;
}

int main() {
    const Case cases[] = {{1280, 720, 8, 1.2f}, {640, 480, 8, 1.2f}, {333, 222, 5, 1.5f}, {100, 100, 1, 1.2f}, {1920, 1080, 12, 1.1f}};
    for (const Case &k : cases) if (!check(k)) return 1;
    std::printf("split ok\n");
    return 0;
}
