// Compile + link check of the triangulator of the host mirror (mi355slam::triangulateMapPoints in mi355slam/map_update.hpp) against
// libmi355slam.so (tests/test_triangulate_abi.py) and its run on one small scene (tests/test_gpu_triangulate.py).
//   triangulate_smoke --no-gpu       the MS_ERR_INVALID cases of ms_triangulate through ms_triangulate_check (no context, no device); this is
//                                    also the stand-alone program the host validation runs under the sanitizers with
//   triangulate_smoke --gpu SCENE    SCENE = a text file the test writes (tests/test_gpu_triangulate.py: write_scene): the tables, the lists,
//                                    the settings and, per mode, what tests/triangulate_ref.py expects.  Drives the mirror once per mode on
//                                    fresh tables and prints one `ok` line per mode.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mi355slam/map_update.hpp"

using namespace mi355slam;

namespace {

// ---- --no-gpu -------------------------------------------------------------------------------------------------------------------------
struct Case {
    int nMp = 10, nKf = 3, mode = MS_TRI_TME;
    std::vector<ms_pinhole> cam{{500, 500, 320, 240, 640, 480}, {500, 500, 320, 240, 640, 480}, {500, 500, 320, 240, 640, 480}};
    std::vector<std::int32_t> focal{500, 500, 500}, rows{4, 2, 9}, start{0, 2, 2, 5}, kf{0, 1, 0, 1, 2}, octave{0, 7, 3, 3, 1};
    std::vector<std::uint8_t> was{0, 1, 0};
    std::vector<float> x{1, 2, 3, 4, 5}, y{1, 2, 3, 4, 5}, sigma{1.f, 1.44f, 2.07f, 2.99f, 4.3f, 6.19f, 8.92f, 12.84f};
    ms_tri_settings s{nullptr, 8, 1.0, 3.0, 0.004f, 0};
};
char why[256];
int cases = 0;

int check(Case &c, const double *pos = reinterpret_cast<const double *>(0x1000), const double *pose = reinterpret_cast<const double *>(0x2000)) {
    why[0] = 0;
    if (!c.s.level_sigma_sq) c.s.level_sigma_sq = c.sigma.data();
    return ms_triangulate_check(pos, c.nMp, pose, c.nKf, c.cam.data(), c.focal.data(), c.rows.data(), c.was.data(), (int)c.rows.size(), c.start.data(), c.kf.data(),
                                c.x.data(), c.y.data(), c.octave.data(), &c.s, c.mode, why, sizeof(why));
}
bool rejected(int rc, const char *what) {
    ++cases;
    if (rc == MS_ERR_INVALID && why[0]) return true;
    std::printf("not rejected (%d, \"%s\"): %s\n", rc, why, what);
    return false;
}

int no_gpu() {
    bool good = true;
    { Case c; if (check(c) != MS_OK) { std::printf("a valid call was rejected: %s\n", why); return 1; } }
    { Case c; c.rows.clear(); c.was.clear(); c.start = {0}; if (check(c, nullptr, nullptr) != MS_OK) { std::printf("n_rows = 0 was rejected: %s\n", why); return 1; } }
    { Case c; c.rows[1] = 10; good &= rejected(check(c), "row beyond the table"); }
    { Case c; c.rows[0] = -1; good &= rejected(check(c), "row -1"); }
    { Case c; c.rows[2] = 4; good &= rejected(check(c), "row listed twice"); }
    { Case c; c.kf[3] = 3; good &= rejected(check(c), "slot beyond the table"); }
    { Case c; c.kf[0] = -1; good &= rejected(check(c), "slot -1"); }
    { Case c; c.start[0] = 1; good &= rejected(check(c), "obs_start[0] != 0"); }
    { Case c; c.start[2] = 1; good &= rejected(check(c), "obs_start decreases"); }
    { Case c; c.octave[1] = 8; good &= rejected(check(c), "octave n_levels"); }
    { Case c; c.octave[4] = -1; good &= rejected(check(c), "octave -1"); }
    { Case c; c.cam[1].width = 0; good &= rejected(check(c), "width 0"); }
    { Case c; c.cam[2].height = 0; good &= rejected(check(c), "height 0"); }
    { Case c; c.cam[0].fx = 0.0; good &= rejected(check(c), "fx 0"); }
    { Case c; c.cam[0].fy = -500.0; good &= rejected(check(c), "fy negative"); }
    { Case c; c.cam[1].fx = NAN; good &= rejected(check(c), "fx NaN"); }
    { Case c; c.mode = 3; good &= rejected(check(c), "mode 3"); }
    { Case c; c.mode = -1; good &= rejected(check(c), "mode -1"); }
    { Case c; c.s.min_angle_two_obs = NAN; good &= rejected(check(c), "NaN angle"); }
    { Case c; c.s.min_angle_multiple_obs = INFINITY; good &= rejected(check(c), "infinite angle"); }
    { Case c; c.s.rel_reprojection_threshold = NAN; good &= rejected(check(c), "NaN threshold"); }
    { Case c; c.sigma[3] = INFINITY; good &= rejected(check(c), "infinite sigma"); }
    { Case c; c.s.n_levels = 0; good &= rejected(check(c), "n_levels 0"); }
    { Case c; c.s.n_levels = MS_TRI_MAX_LEVELS + 1; good &= rejected(check(c), "n_levels beyond the cap"); }
    { Case c; c.nMp = -1; good &= rejected(check(c), "negative n_mp"); }
    { Case c; good &= rejected(check(c, nullptr), "missing positions"); }
    { Case c; good &= rejected(check(c, reinterpret_cast<const double *>(0x1000), nullptr), "missing poses"); }
    {
        Case c;
        c.s.level_sigma_sq = c.sigma.data();
        why[0] = 0;
        good &= rejected(ms_triangulate_check(reinterpret_cast<const double *>(0x1000), c.nMp, reinterpret_cast<const double *>(0x2000), c.nKf, c.cam.data(), c.focal.data(),
                                              c.rows.data(), c.was.data(), 3, c.start.data(), nullptr, c.x.data(), c.y.data(), c.octave.data(), &c.s, c.mode, why, sizeof(why)),
                         "missing obs_kf");
        why[0] = 0;
        good &= rejected(ms_triangulate_check(reinterpret_cast<const double *>(0x1000), c.nMp, reinterpret_cast<const double *>(0x2000), c.nKf, c.cam.data(), c.focal.data(),
                                              c.rows.data(), c.was.data(), 3, c.start.data(), c.kf.data(), c.x.data(), c.y.data(), c.octave.data(), nullptr, c.mode, why, sizeof(why)),
                         "missing settings");
    }
    if (!good) return 1;
    std::printf("no-gpu ok %d cases\n", cases);
    return 0;
}

// ---- --gpu ----------------------------------------------------------------------------------------------------------------------------
struct Reader {
    std::FILE *f;
    bool good = true;
    double d() { char t[64]; if (std::fscanf(f, "%63s", t) != 1) { good = false; return 0; } return std::strtod(t, nullptr); }
    long i() { long v = 0; if (std::fscanf(f, "%ld", &v) != 1) good = false; return v; }
    template <class T> std::vector<T> ints(std::size_t n) { std::vector<T> v(n); for (auto &e : v) e = (T)i(); return v; }
    std::vector<float> floats(std::size_t n) { std::vector<float> v(n); for (auto &e : v) e = (float)d(); return v; }
};

int gpu(const char *path) {
    Reader in{std::fopen(path, "r")};
    if (!in.f) { std::printf("cannot read %s\n", path); return 2; }
    const std::size_t nKf = in.i(), nMp = in.i(), nRows = in.i(), nObs = in.i(), nLevels = in.i();
    const bool hasDepth = in.i() != 0;
    Parameters p;
    p.orbScaleLevels = (unsigned)nLevels;
    p.minTriangulationAngleTwoObs = in.d(); p.minTriangulationAngleMultipleObs = in.d(); p.relativeReprojectionErrorThreshold = (float)in.d();
    const double tolerance = in.d();
    StaticSettings settings(p);
    std::vector<DeviceKeyframePoses::Pose> poses(nKf);
    for (auto &P : poses) for (double &v : P) v = in.d();
    KeyframeSlots cams;
    for (std::size_t k = 0; k < nKf; ++k) {
        ms_pinhole c;
        c.fx = in.d(); c.fy = in.d(); c.cx = in.d(); c.cy = in.d(); c.width = (std::int32_t)in.d(); c.height = (std::int32_t)in.d();
        cams.camera.push_back(c);
    }
    cams.focalLength = in.ints<std::int32_t>(nKf);
    settings.levelSigmaSq = in.floats(nLevels);
    std::vector<DeviceMapPoints::Vec3d> pos(nMp);
    for (auto &v : pos) for (double &e : v) e = in.d();
    const std::vector<std::uint8_t> flags0 = in.ints<std::uint8_t>(nMp);
    TriangulateArgs args;
    args.rows = in.ints<std::int32_t>(nRows);
    args.wasTriangulated = in.ints<std::uint8_t>(nRows);
    args.obsStart = in.ints<std::int32_t>(nRows + 1);
    args.obsKf = in.ints<std::int32_t>(nObs);
    args.obsX = in.floats(nObs); args.obsY = in.floats(nObs);
    args.obsOctave = in.ints<std::int32_t>(nObs);
    if (hasDepth) args.obsDepth = in.floats(nObs);
    if (!in.good) { std::printf("%s is cut short\n", path); return 2; }

    Context ctx(0);
    DeviceKeyframePoses dposes(ctx, poses);
    const std::vector<DeviceMapPoints::Vec3f> norm(nMp, DeviceMapPoints::Vec3f{0.f, 0.f, 1.f});
    const std::vector<float> dist(nMp, 1.f);
    const std::vector<KeyPoint::Descriptor> desc(nMp, KeyPoint::Descriptor{});
    const char *names[3] = {"TME", "MIDPOINT", "FIRST_LAST"};
    for (int mode = 0; mode < 3; ++mode) {
        const std::vector<std::uint8_t> wStatus = in.ints<std::uint8_t>(nRows), wReason = in.ints<std::uint8_t>(nRows);
        const std::vector<std::int32_t> wPass = in.ints<std::int32_t>(nRows);
        const std::vector<std::uint8_t> wFlags = in.ints<std::uint8_t>(nMp);
        std::vector<double> wPos(3 * nMp);
        for (double &v : wPos) v = in.d();
        if (!in.good) { std::printf("%s is cut short (mode %d)\n", path, mode); return 2; }
        DeviceMapPoints table(ctx, pos, norm, dist, dist, desc);
        DeviceMapPointFlags flags(ctx, flags0);
        const TriangulateResult got = triangulateMapPoints(ctx, table, &flags, dposes, cams, args, settings, (TriangulationMethod)mode);
        if (got.status != wStatus || got.reason != wReason || got.passCount != wPass) { std::printf("%s: status, reason or pass count differ\n", names[mode]); return 3; }
        std::vector<std::uint8_t> gFlags(nMp);
        std::vector<double> gPos(3 * nMp);
        ctx.check(ms_dev_download(ctx.get(), gFlags.data(), flags.flags(), nMp), "ms_dev_download");
        ctx.check(ms_dev_download(ctx.get(), gPos.data(), table.position(), 24 * nMp), "ms_dev_download");
        if (gFlags != wFlags) { std::printf("%s: flags differ\n", names[mode]); return 4; }
        double worst = 0.0;
        std::size_t triangulated = 0;
        std::vector<std::uint8_t> succeeded(nMp, 0);         // only a row that triangulated may differ within the tolerance
        for (std::size_t i = 0; i < nRows; ++i) succeeded[args.rows[i]] = wStatus[i] != 0;
        for (std::size_t r = 0; r < nMp; ++r) {
            if (!succeeded[r] && std::memcmp(&gPos[3 * r], &wPos[3 * r], 24) != 0) { std::printf("%s: row %zu (untouched or failed) is not bit-equal\n", names[mode], r); return 5; }
            double diff = 0.0, size = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double g = gPos[3 * r + k], w = wPos[3 * r + k];
                if (std::isfinite(g) != std::isfinite(w)) { std::printf("%s: row %zu is finite on one side only\n", names[mode], r); return 5; }
                if (std::isfinite(w)) { diff = std::max(diff, std::fabs(g - w)); size = std::max(size, std::fabs(w)); }
            }
            if (diff > tolerance * size) { std::printf("%s: row %zu differs by %.3e relative\n", names[mode], r, diff / size); return 5; }
            if (size > 0.0) worst = std::max(worst, diff / size);
        }
        for (std::uint8_t s : got.status) triangulated += s != 0;
        std::printf("ok %s %zu rows %zu triangulated worst relative difference %.3e\n", names[mode], nRows, triangulated, worst);
    }
    std::fclose(in.f);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    // referencing the entry points makes the link fail if the library does not export them
    volatile const void *syms[] = {(const void *)&ms_triangulate, (const void *)&ms_triangulate_check};
    std::printf("link ok %d\n", syms[0] != nullptr && syms[1] != nullptr);
    if (argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0) return no_gpu();
    if (argc > 2 && std::strcmp(argv[1], "--gpu") == 0) return gpu(argv[2]);
    return 0;
}
