// The handle's plan (stereo_matching_amd/csrc/sgm_plan.h: the parameter check
// and the schedule sgm_create picks) on the CPU, for a sanitizer build:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all plan_main.cpp
// One line of output per argument, each argument one row:
//   plan:H,W,S,D,VIEWS,PATHS,CUS[,NAME=VALUE...]   the plan of sgm_default_params(H, W, S, D) with
//       views and paths as given on a device of CUS compute units, under the switches NAME=VALUE
//       (SGM_SLANT, SGM_VSTRIP, SGM_BAND_ROWS, SGM_P4_HPAIR) and no others, and after it the plan
//       again without the slanted schedule (plan_without_slant)
//   params:H,W,S,D[,FIELD=VALUE...]   valid_params of sgm_default_params(H, W, S, D) with the
//       fields of sgm_params as given: "ok", or "refused: " and the message
// tests/test_plan_cpu.py holds the rows and what they must print.
#include "../../stereo_matching_amd/csrc/sgm_plan.h"

#include <string.h>
#include <string>
#include <vector>

static std::vector<std::string> split(const std::string &s) {
    std::vector<std::string> out;
    size_t a = 0;
    for (size_t b; (b = s.find(',', a)) != std::string::npos; a = b + 1) out.push_back(s.substr(a, b - a));
    out.push_back(s.substr(a));
    return out;
}

// NAME=VALUE: true when the name is `name`, the value in *value
static bool setting(const std::string &kv, const char *name, std::string *value) {
    const size_t n = strlen(name);
    if (kv.compare(0, n, name) != 0 || kv.size() <= n || kv[n] != '=') return false;
    *value = kv.substr(n + 1);
    return true;
}

static const char *sched_name(sgm::Schedule s) {
    switch (s) {
    case sgm::SCHED_PATHS4: return "PATHS4";
    case sgm::SCHED_SLANT: return "SLANT";
    case sgm::SCHED_JOINT: return "JOINT";
    case sgm::SCHED_BANDS: return "BANDS";
    case sgm::SCHED_WHOLE_FINAL2: return "WHOLE_FINAL2";
    case sgm::SCHED_PER_VIEW: return "PER_VIEW";
    }
    return "?";
}

static void print_plan(const sgm::HandlePlan &p) {
    printf("H=%d W=%d D=%d scale=%d nviews=%d paths4=%d p4_split=%d slant=%d slant_forced=%d vstrip=%d "
           "band_rows=%d sched=%s sub_cm=%d",
           p.g.H, p.g.W, p.g.D, p.g.scale, p.nviews, p.paths4, p.p4_split, p.slant, p.slant_forced, p.vstrip,
           p.band_rows, sched_name(p.sched), p.sub_cm);
}

static bool plan_row(const std::vector<std::string> &f) {
    if (f.size() < 7) return false;
    sgm_params p;
    sgm::default_params(&p, atoi(f[0].c_str()), atoi(f[1].c_str()), atoi(f[2].c_str()), atoi(f[3].c_str()));
    p.views = atoi(f[4].c_str());
    p.paths = atoi(f[5].c_str());
    const int cus = atoi(f[6].c_str());
    sgm::PlanEnv env;
    for (size_t k = 7; k < f.size(); ++k)
        if (!setting(f[k], "SGM_SLANT", &env.slant) && !setting(f[k], "SGM_VSTRIP", &env.vstrip) &&
            !setting(f[k], "SGM_BAND_ROWS", &env.band_rows) && !setting(f[k], "SGM_P4_HPAIR", &env.p4_hpair))
            return false;
    char why[256];
    if (!sgm::valid_params(&p, why, sizeof(why))) return false;  // (plan_handle takes accepted parameters)
    const sgm::HandlePlan plan = sgm::plan_handle(p, cus, env);
    print_plan(plan);
    printf(" | without_slant: ");
    print_plan(sgm::plan_without_slant(plan));
    printf("\n");
    return true;
}

static bool params_row(const std::vector<std::string> &f) {
    if (f.size() < 4) return false;
    sgm_params p;
    sgm::default_params(&p, atoi(f[0].c_str()), atoi(f[1].c_str()), atoi(f[2].c_str()), atoi(f[3].c_str()));
    const struct { const char *name; int *field; } ints[] = {
        {"p1", &p.p1}, {"p2", &p.p2}, {"blur", &p.blur}, {"views", &p.views}, {"post_filter", &p.post_filter},
        {"lk_refine", &p.lk_refine}, {"sky_detect", &p.sky_detect}, {"solver", &p.solver},
        {"aux_only", &p.aux_only}, {"view", &p.view}, {"paths", &p.paths}};
    for (size_t k = 4; k < f.size(); ++k) {
        std::string v;
        bool known = false;
        if (setting(f[k], "uniqueness", &v)) {
            p.uniqueness = (float)atof(v.c_str());
            known = true;
        }
        for (const auto &i : ints)
            if (!known && setting(f[k], i.name, &v)) {
                *i.field = atoi(v.c_str());
                known = true;
            }
        if (!known) return false;
    }
    char why[256];
    if (sgm::valid_params(&p, why, sizeof(why))) printf("ok\n");
    else printf("refused: %s\n", why);
    return true;
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        const std::string row = argv[a];
        bool ok = false;
        if (row.compare(0, 5, "plan:") == 0) ok = plan_row(split(row.substr(5)));
        else if (row.compare(0, 7, "params:") == 0) ok = params_row(split(row.substr(7)));
        if (!ok) {
            fprintf(stderr, "bad row: %s\n", row.c_str());
            return 2;
        }
    }
    return 0;
}
