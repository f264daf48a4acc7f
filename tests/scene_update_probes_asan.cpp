// Stand-alone check of vrt_scene_update_probes' host-only path for a sanitizer
// run on a machine without a GPU: a host-only probe scene (device < 0) is
// created, updated to moved positions and probes, compared array for array
// with a scene freshly created from them, updated back (probes = NULL, then
// with the first probes) and compared with the original; the stored SGs stay;
// then the refusals that need no device.  Not part of the pytest suite.  Built
// by the recipe in the header of tests/scene_update_asan.cpp with this file in
// place of that one.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "vrt.h"

static uint32_t rng_state = 4321u;
static float frand()
{
        rng_state = rng_state * 1664525u + 1013904223u;
        return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

struct Snapshot {
        vrt_scene_info_t info;
        int32_t rec = 0, nprobe = 0;
        int64_t pleaves = 0, prefs = 0;
        std::vector<float> box;
        std::vector<uint32_t> a, b, vox, cnt, pvox, pcnt;
        std::vector<int32_t> tris, probes;
};

static int fails = 0;
#define CHECK(c)                                                                  \
        do {                                                                      \
                if (!(c)) {                                                       \
                        std::printf("FAILED line %d: %s (%s)\n", __LINE__, #c, vrt_last_error()); \
                        ++fails;                                                  \
                }                                                                 \
        } while (0)

static Snapshot snap(vrt_scene *s)
{
        Snapshot q;
        CHECK(vrt_scene_info(s, &q.info) == VRT_OK);
        CHECK(vrt_scene_ref_format(s, &q.rec) == VRT_OK);
        const size_t n = (size_t)q.info.nodes;
        q.box.resize(6 * n);
        q.a.resize(n);
        q.b.resize(n);
        CHECK(vrt_scene_nodes(s, q.box.data(), q.a.data(), q.b.data()) == VRT_OK);
        q.vox.resize((size_t)q.info.nonempty_leaves + 1);
        q.cnt.resize((size_t)q.info.nonempty_leaves + 1);
        q.tris.resize((size_t)q.info.tri_refs + 1);
        CHECK(vrt_scene_leaves(s, q.vox.data(), q.cnt.data(), q.tris.data()) == VRT_OK);
        CHECK(vrt_scene_probe_info(s, &q.nprobe, &q.pleaves, &q.prefs) == VRT_OK);
        q.pvox.resize((size_t)q.pleaves + 1);
        q.pcnt.resize((size_t)q.pleaves + 1);
        q.probes.resize((size_t)q.prefs + 1);
        CHECK(vrt_scene_probe_leaves(s, q.pvox.data(), q.pcnt.data(), q.probes.data()) == VRT_OK);
        return q;
}

static bool same(const Snapshot &x, const Snapshot &y)
{
        return x.info.nodes == y.info.nodes && x.info.internal == y.info.internal && x.info.leaves == y.info.leaves &&
               x.info.nonempty_leaves == y.info.nonempty_leaves && x.info.tri_refs == y.info.tri_refs &&
               !std::memcmp(x.info.root_min, y.info.root_min, 12) && !std::memcmp(x.info.root_max, y.info.root_max, 12) &&
               x.rec == y.rec && x.box.size() == y.box.size() &&
               !std::memcmp(x.box.data(), y.box.data(), x.box.size() * 4) && x.a == y.a && x.b == y.b &&
               x.vox == y.vox && x.cnt == y.cnt && x.tris == y.tris && x.nprobe == y.nprobe &&
               x.pleaves == y.pleaves && x.prefs == y.prefs && x.pvox == y.pvox && x.pcnt == y.pcnt &&
               x.probes == y.probes;
}

int main()
{
        const int n = 500, depth = 5, np = 9;
        std::vector<float> pos((size_t)n * 9), nrm((size_t)n * 9), moved((size_t)n * 9);
        for (int i = 0; i < n; ++i) {
                const float c[3] = { frand(), frand(), frand() };
                for (int v = 0; v < 3; ++v)
                        for (int k = 0; k < 3; ++k) {
                                pos[9 * i + 3 * v + k] = c[k] + 0.1f * (frand() - 0.5f);
                                nrm[9 * i + 3 * v + k] = k == 1 ? 2.f : 0.25f;
                        }
        }
        const float cs = std::cos(0.4f), sn = std::sin(0.4f);
        for (int j = 0; j < 3 * n; ++j) {
                const float *p = &pos[3 * j];
                moved[3 * j + 0] = cs * p[0] + sn * p[2] + 0.5f;
                moved[3 * j + 1] = p[1] - 0.25f;
                moved[3 * j + 2] = -sn * p[0] + cs * p[2];
        }
        // probes inside, across a face and outside the triangles' box, one with
        // r = 0; moved with the triangles, with other radii (one dies, one wakes)
        std::vector<vrt_probe> pr(np), pm(np);
        for (int k = 0; k < np; ++k) {
                pr[k] = { { frand(), frand(), frand() }, 0.02f + 0.1f * frand() };
                if (k == 7)
                        pr[k] = { { 1.6f, 1.5f, 1.4f }, 0.1f };
                if (k == 8)
                        pr[k].r = 0.f;
                pm[k].o[0] = cs * pr[k].o[0] + sn * pr[k].o[2] + 0.5f;
                pm[k].o[1] = pr[k].o[1] - 0.25f;
                pm[k].o[2] = -sn * pr[k].o[0] + cs * pr[k].o[2];
                pm[k].r = k == 2 ? 0.f : k == 8 ? 0.07f : 1.5f * pr[k].r;
        }
        const int32_t mat_tex[1] = { -1 };
        const float mat_kd[3] = { 0.8f, 0.8f, 0.8f };
        vrt_scene_desc d{};
        d.ntri = n;
        d.pos = pos.data();
        d.nrm = nrm.data();
        d.nmat = 1;
        d.mat_tex = mat_tex;
        d.mat_kd = mat_kd;
        vrt_scene *s = nullptr, *orig = nullptr, *fresh = nullptr, *half = nullptr;
        CHECK(vrt_scene_create_probes(&d, pr.data(), np, depth, -1, 0, &s) == VRT_OK);
        CHECK(vrt_scene_create_probes(&d, pr.data(), np, depth, -1, 0, &orig) == VRT_OK);
        vrt_scene_desc dm = d;
        dm.pos = moved.data();
        CHECK(vrt_scene_create_probes(&dm, pm.data(), np, depth, -1, 0, &fresh) == VRT_OK);
        CHECK(vrt_scene_create_probes(&d, pm.data(), np, depth, -1, 0, &half) == VRT_OK);
        const Snapshot q0 = snap(orig), q1 = snap(fresh), qh = snap(half);
        CHECK(!same(q0, q1) && !same(q0, qh) && q1.prefs > 0);
        // the stored SGs are the caller's and stay
        std::vector<vrt_sg> sgs((size_t)VRT_PROBE_SGS * np), got(sgs.size());
        for (size_t i = 0; i < sgs.size() * sizeof(vrt_sg) / sizeof(float); ++i)
                reinterpret_cast<float *>(sgs.data())[i] = frand();
        CHECK(vrt_scene_set_probe_sgs(s, sgs.data()) == VRT_OK);
        CHECK(vrt_scene_update_probes(s, moved.data(), nrm.data(), pm.data()) == VRT_OK);
        CHECK(same(snap(s), q1));
        CHECK(vrt_scene_probe_sgs(s, got.data()) == VRT_OK);
        CHECK(!std::memcmp(got.data(), sgs.data(), sgs.size() * sizeof(vrt_sg)));
        double ms[4];
        CHECK(vrt_scene_update_stats(s, ms) == VRT_OK && ms[0] > 0);
        CHECK(vrt_scene_update_probes(s, pos.data(), nullptr, nullptr) == VRT_OK);  // only the triangles move
        CHECK(same(snap(s), qh));
        CHECK(vrt_scene_update_probes(s, pos.data(), nullptr, pr.data()) == VRT_OK);
        CHECK(same(snap(s), q0));
        // refusals: the scene stays as it is
        CHECK(vrt_scene_update_probes(s, nullptr, nullptr, pm.data()) == VRT_E_INVALID);
        CHECK(vrt_scene_update_probes(nullptr, pos.data(), nullptr, pm.data()) == VRT_E_INVALID);
        CHECK(vrt_scene_update_probes_device(s, pos.data(), nullptr, nullptr, nullptr) == VRT_E_NODEVICE);
        CHECK(vrt_scene_update(s, moved.data(), nullptr) == VRT_E_INVALID);
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        const vrt_probe bad[3] = { { { nan, 0.5f, 0.5f }, 0.1f }, { { 0.5f, 0.5f, 0.5f }, -0.25f },
                                   { { 0.5f, 0.5f, 0.5f }, inf } };
        for (int i = 0; i < 3; ++i) {
                std::vector<vrt_probe> q = pm;
                q[3 + i] = bad[i];
                CHECK(vrt_scene_update_probes(s, moved.data(), nullptr, q.data()) == VRT_E_INVALID);
                char want[16];
                std::snprintf(want, sizeof want, "probe %d:", 3 + i);
                CHECK(std::strstr(vrt_last_error(), want) != nullptr);
        }
        vrt_scene *plain = nullptr;
        CHECK(vrt_scene_create(&d, depth, -1, &plain) == VRT_OK);
        CHECK(vrt_scene_update_probes(plain, moved.data(), nullptr, nullptr) == VRT_E_INVALID);
        CHECK(std::strstr(vrt_last_error(), "vrt_scene_update") != nullptr);
        CHECK(same(snap(s), q0));
        for (int i = 0; i < 5; ++i)
                CHECK(vrt_scene_update_probes(s, i % 2 ? pos.data() : moved.data(), nrm.data(),
                                              i % 2 ? pr.data() : pm.data()) == VRT_OK);
        CHECK(same(snap(s), q1));
        vrt_scene_destroy(plain);
        vrt_scene_destroy(s);
        vrt_scene_destroy(orig);
        vrt_scene_destroy(fresh);
        vrt_scene_destroy(half);
        std::printf(fails ? "scene_update_probes_asan: %d check(s) failed\n" : "scene_update_probes_asan: ok\n", fails);
        return fails ? 1 : 0;
}
