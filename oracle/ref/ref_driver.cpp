/*
 * ref_driver.cpp -- runs the reference's own SGM / BM / Solver code on a
 * request file and writes what it computed, stage by stage, as raw arrays.
 *
 * TEST INFRASTRUCTURE ONLY.  oracle/Makefile (target ref) compiles this file
 * together with the reference's unmodified src/{Solver,SGM,cost,BM}.cpp
 * against the stand-in headers in oracle/ref/include/ into oracle/_ref/,
 * which stays out of version control.  tests/golden/make_ref_golden.py turns
 * the output into the ref_* fixtures.
 *
 * The driver names the reference's members and methods and restates none of
 * their bodies.  It is compiled with -fno-access-control, so it can read the
 * protected (Solver) and private (SGM) members.  It defines what the four
 * reference files leave undefined:
 *   - get_cur_ms() (src/utils.cpp is not compiled).  SGM::process, BM::process
 *     and Solver::post_filter call it between their stages, so here it is the
 *     snapshot hook: every call dumps the state the stage before it left
 *     behind (see snapshot_sgm / snapshot_bm for which call is which).  That
 *     makes every stage inside process() visible without editing it.
 *   - LKSubPixel's constructor, destructor and create() (returns null: the
 *     LKRefine call at SGM.cpp:824 is commented out, Solver only stores it).
 *   - cv::GaussianBlur, as identity or as DESIGN.md's pinned fixed-point
 *     formula (written here afresh), chosen by the request; cv::cvtColor is
 *     only linked, never called.
 *
 * Request (little-endian): int32 magic, mode, h, w, scale, D, blur, has_sky,
 * has_map, reserved; u8 left[h*w], right[h*w]; if has_sky u8 sky_l[H*W],
 * sky_r[H*W]; if has_map f32 map[H*W]  (H = h/scale, W = w/scale).
 * Output: records of char name[16], int32 kind (0 u8, 1 f32, 2 u64),
 * int32 d0, d1, d2 (d2 = 0: two-dimensional), then the bytes.
 *
 * usage: ref_driver REQUEST OUTPUT
 */
#include <inc/SGM.h>
#include <inc/BM.h>

enum { MODE_STAGES = 0, MODE_PROCESS = 1, MODE_BM = 2, MODE_POST_FILTER = 3, MODE_SUBPIXEL = 4,
       MODE_COLORMAP = 5 };
enum { KIND_U8 = 0, KIND_F32 = 1, KIND_U64 = 2 };

static FILE *g_out = NULL;
static Solver *g_solver = NULL;   /* non-null: get_cur_ms() snapshots it */
static int g_mode = 0, g_calls = 0, g_blur = 0;

/* ------------------------------------------------------------- output */

static void put(const char *name, int kind, const void *p, int d0, int d1, int d2)
{
    static const size_t esz[3] = {1, 4, 8};
    char nm[16];
    std::memset(nm, 0, sizeof nm);
    std::strncpy(nm, name, sizeof nm - 1);
    int32_t hd[4] = {kind, d0, d1, d2};
    size_t n = (size_t)d0 * (size_t)d1 * (size_t)(d2 ? d2 : 1) * esz[kind];
    if (fwrite(nm, 1, sizeof nm, g_out) != sizeof nm || fwrite(hd, sizeof hd, 1, g_out) != 1 ||
        fwrite(p, 1, n, g_out) != n) {
        fprintf(stderr, "ref_driver: short write\n");
        exit(2);
    }
}

static void put_mat(const char *name, const Mat &m)
{
    const int ch = m.channels();
    put(name, m.depth() == CV_32F ? KIND_F32 : KIND_U8, m.data, m.rows, m.cols, ch > 1 ? ch : 0);
}

static void put_vol(const char *name, const Solver *s, const float *v)
{
    put(name, KIND_F32, v, s->img_h, s->img_w, s->max_disp);
}

static void put_paths(SGM *s, const char *suffix)
{
    float *L[8] = {s->L1, s->L2, s->L3, s->L4, s->L5, s->L6, s->L7, s->L8};
    for (int k = 0; k < 8; ++k) {
        char nm[16];
        snprintf(nm, sizeof nm, "L%d%s", k + 1, suffix);
        put_vol(nm, s, L[k]);
    }
}

/* --------------------------------------------------- snapshot hook */

/* get_cur_ms() calls inside SGM::process (src/SGM.cpp) and the post_filter it
 * ends with (src/Solver.cpp:602,635), in order:
 *   1 :65 before build_cost_table     2 :68 after build_dsi_from_table
 *   3 :70 before the cost filters     4 :73 after both filters
 *   5 :75 before L1                   6 :421 after aggregation + WTA
 *   7 :448 after compute_subpixel     8 :450 after build_dsi_from_table_beta
 *   9 :452                           10 :455 after both filters (beta)
 *  11 :457                           12 :799 after aggregation + WTA (beta)
 *  13 Solver.cpp:602, post_filter's first line: sub-pixel (beta) and the LR
 *     loop are done                  14 Solver.cpp:635 after the speckle filter */
static void snapshot_sgm(SGM *s, int call)
{
    const int n = s->img_h * s->img_w;
    (void)n;
    switch (call) {
    case 1:
        put_mat("img_l", s->img_l);
        put_mat("img_r", s->img_r);
        break;
    case 2:
        put("ct_l", KIND_U64, s->cost_table_l, s->img_h, s->img_w, 0);
        put("ct_r", KIND_U64, s->cost_table_r, s->img_h, s->img_w, 0);
        put_vol("dsi", s, s->cost);
        break;
    case 4: put_vol("vf", s, s->cost); break;
    case 6:
        put_paths(s, "");
        put_vol("S", s, s->cost);
        put_mat("disp", s->disp);
        break;
    case 7: put_mat("sub", s->filtered_disp); break;
    case 8: put_vol("dsi_b", s, s->cost); break;
    case 10: put_vol("vf_b", s, s->cost); break;
    case 12:
        put_paths(s, "_b");
        put_vol("S_b", s, s->cost);
        put_mat("disp_b", s->disp_beta);
        break;
    case 13:
        put_mat("sub_b", s->filtered_disp_beta);
        put_mat("lr", s->filtered_disp);
        break;
    default: break;
    }
}

/* BM::process (src/BM.cpp): 1 :40, 2 :43 after build_dsi_from_table, 3 :45,
 * 4 :48 after both filters, 5 :50, 6 :94 after the WTA, 7/8 post_filter. */
static void snapshot_bm(BM *s, int call)
{
    switch (call) {
    case 1:
        put_mat("img_l", s->img_l);
        put_mat("img_r", s->img_r);
        break;
    case 2:
        put("ct_l", KIND_U64, s->cost_table_l, s->img_h, s->img_w, 0);
        put("ct_r", KIND_U64, s->cost_table_r, s->img_h, s->img_w, 0);
        break;
    case 4: put_vol("vf", s, s->cost); break;
    case 6: put_mat("disp", s->disp); break;
    default: break;
    }
}

double get_cur_ms()
{
    ++g_calls;
    /* post_filter()'s first line (call 13 of SGM::process, 7 of BM::process):
     * speckle_filter_new's union-find races between OpenMP threads
     * (Solver.cpp:525-546) and a racing Find can loop for ever, so from here
     * on the run has one thread.  Everything before it is deterministic. */
    if (g_calls == (g_mode == MODE_BM ? 7 : 13) &&
        (g_mode == MODE_BM || g_mode == MODE_PROCESS || g_mode == MODE_SUBPIXEL))
        omp_set_num_threads(1);
    if (g_solver) {
        if (g_mode == MODE_PROCESS)
            snapshot_sgm(static_cast<SGM *>(g_solver), g_calls);
        else if (g_mode == MODE_BM)
            snapshot_bm(static_cast<BM *>(g_solver), g_calls);
    }
    return 0.0;
}

/* ------------------------------------------- what the reference leaves open */

LKSubPixel::LKSubPixel(int, int, int, int) {}
LKSubPixel::~LKSubPixel() {}
std::shared_ptr<LKSubPixel> LKSubPixel::create(int, int, int, int) { return std::shared_ptr<LKSubPixel>(); }

static int reflect101(int i, int n)
{
    if (n == 1)
        return 0;
    while (i < 0 || i >= n)
        i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

namespace cv {

/* Only the call the reference makes: Size(3,3), sigmaX 2, sigmaY 1
 * (Solver.cpp:124-125).  g_blur 0: identity.  g_blur 1: DESIGN.md's pinned
 * formula -- row taps {82,93,82}, column taps {70,116,70}, BORDER_REFLECT_101,
 * (acc + 2^15) >> 16, saturated to 8 bits.  OpenCV's own arithmetic stays
 * unpinned: it is not on this machine. */
void GaussianBlur(const Mat &src, Mat &dst, Size ksize, double sigmaX, double sigmaY)
{
    assert(ksize.width == 3 && ksize.height == 3 && sigmaX == 2 && sigmaY == 1);
    assert(src.type() == CV_8UC1);
    const int H = src.rows, W = src.cols;
    Mat out(H, W, CV_8UC1);
    if (!g_blur) {
        src.copyTo(out);
    } else {
        const int tx[3] = {82, 93, 82}, ty[3] = {70, 116, 70};
        for (int i = 0; i < H; ++i)
            for (int j = 0; j < W; ++j) {
                int acc = 0;
                for (int a = 0; a < 3; ++a) {
                    const uchar *row = src.ptr<uchar>(reflect101(i + a - 1, H));
                    int r = 0;
                    for (int b = 0; b < 3; ++b)
                        r += tx[b] * row[reflect101(j + b - 1, W)];
                    acc += ty[a] * r;
                }
                const int v = (acc + (1 << 15)) >> 16;
                out.at<uchar>(i, j) = (uchar)(v > 255 ? 255 : v);
            }
    }
    dst = out;
}

void cvtColor(const Mat &, Mat &, int) { abort(); }

} /* namespace cv */

/* ------------------------------------------------------------ request */

struct Request {
    int32_t mode, h, w, scale, D, blur, has_sky, has_map;
    std::vector<uchar> left, right, sky_l, sky_r;
    std::vector<float> map;
};

static void need(bool ok, const char *what)
{
    if (!ok) {
        fprintf(stderr, "ref_driver: bad request (%s)\n", what);
        exit(2);
    }
}

static Request read_request(const char *path)
{
    Request q;
    FILE *f = fopen(path, "rb");
    need(f != NULL, "open");
    int32_t hd[10];
    need(fread(hd, sizeof hd, 1, f) == 1 && hd[0] == 0x51524753, "header");
    q.mode = hd[1]; q.h = hd[2]; q.w = hd[3]; q.scale = hd[4]; q.D = hd[5];
    q.blur = hd[6]; q.has_sky = hd[7]; q.has_map = hd[8];
    need(q.h > 0 && q.w > 0 && q.h <= 4096 && q.w <= 8192 && (q.scale == 1 || q.scale == 2), "sizes");
    const size_t n = (size_t)q.h * q.w, N = (size_t)(q.h / q.scale) * (q.w / q.scale);
    q.left.resize(n);
    q.right.resize(n);
    need(fread(q.left.data(), 1, n, f) == n && fread(q.right.data(), 1, n, f) == n, "images");
    if (q.has_sky) {
        q.sky_l.resize(N);
        q.sky_r.resize(N);
        need(fread(q.sky_l.data(), 1, N, f) == N && fread(q.sky_r.data(), 1, N, f) == N, "sky");
    }
    if (q.has_map) {
        q.map.resize(N);
        need(fread(q.map.data(), 4, N, f) == N, "map");
    }
    fclose(f);
    return q;
}

static void load_map(Solver &s, const Request &q)
{
    need(q.has_map, "map missing");
    for (int i = 0; i < s.img_h; ++i)
        for (int j = 0; j < s.img_w; ++j) {
            const float v = q.map[(size_t)i * s.img_w + j];
            s.filtered_disp.at<float>(i, j) = v;
            s.disp.at<uchar>(i, j) = (uchar)(v < 0 ? 0 : v > 255 ? 255 : v);
        }
}

/* One view of the stages mode: the cost after build_dsi_from_table[_beta],
 * after cost_horizontal_filter and after cost_vertical_filter. */
static void stage_view(SGM &s, bool beta)
{
    if (beta)
        s.build_dsi_from_table_beta();
    else
        s.build_dsi_from_table();
    put_vol(beta ? "dsi_b" : "dsi", &s, s.cost);
    s.cost_horizontal_filter(COST_WIN_W / s.scale);
    put_vol(beta ? "hf_b" : "hf", &s, s.cost);
    s.cost_vertical_filter(COST_WIN_H / s.scale);
    put_vol(beta ? "vf_b" : "vf", &s, s.cost);
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: ref_driver REQUEST OUTPUT\n");
        return 2;
    }
    Request q = read_request(argv[1]);
    g_out = fopen(argv[2], "wb");
    need(g_out != NULL, "output");
    g_mode = q.mode;
    g_blur = q.blur;
    const int H = q.h / q.scale, W = q.w / q.scale;

    Mat left(q.h, q.w, CV_8UC1, q.left.data()), right(q.h, q.w, CV_8UC1, q.right.data());
    Mat sky_l, sky_r;
    if (q.has_sky) {
        sky_l = Mat(H, W, CV_8UC1, q.sky_l.data());
        sky_r = Mat(H, W, CV_8UC1, q.sky_r.data());
    }

    if (q.mode == MODE_BM) {
        BM s(q.h, q.w, q.scale, q.D);
        g_solver = &s;
        if (q.has_sky)
            s.process(left, right, sky_l, sky_r);
        else
            s.process(left, right);
        g_solver = NULL;
        /* BM never writes filtered_disp (BM.cpp:88 filters what Solver.cpp:20
         * allocated); with the stand-in's zero-filled create() this is
         * post_filter() of a map of zeros, not a value the reference defines. */
        put_mat("get_disp", s.get_disp());
    } else {
        SGM s(q.h, q.w, q.scale, q.D);
        switch (q.mode) {
        case MODE_STAGES:
            /* the decimation of SGM.cpp:40-61 lives inside process(); this is
             * the driver's own statement of it, and the process mode's img_l,
             * img_r snapshots are what pins it */
            s.img_l.create(H, W, CV_8UC1);
            s.img_r.create(H, W, CV_8UC1);
            for (int i = 0; i < H; ++i)
                for (int j = 0; j < W; ++j) {
                    s.img_l.at<uchar>(i, j) = left.at<uchar>(i * q.scale, j * q.scale);
                    s.img_r.at<uchar>(i, j) = right.at<uchar>(i * q.scale, j * q.scale);
                }
            s.sky_mask = sky_l;
            s.sky_mask_beta = sky_r;
            put_mat("img_l", s.img_l);
            put_mat("img_r", s.img_r);
            s.build_cost_table();
            put("ct_l", KIND_U64, s.cost_table_l, H, W, 0);
            put("ct_r", KIND_U64, s.cost_table_r, H, W, 0);
            stage_view(s, false);
            stage_view(s, true);
            break;
        case MODE_PROCESS:
            g_solver = &s;
            if (q.has_sky)
                s.process(left, right, sky_l, sky_r);
            else
                s.process(left, right);
            g_solver = NULL;
            put_mat("final", s.get_disp());
            break;
        case MODE_SUBPIXEL:
            /* process() leaves the right view's aggregated volume in `cost`;
             * compute_subpixel() then runs on it with the given disparities */
            if (q.has_sky)
                s.process(left, right, sky_l, sky_r);
            else
                s.process(left, right);
            load_map(s, q);
            s.compute_subpixel(s.disp, s.filtered_disp);
            put_mat("subpixel", s.filtered_disp);
            break;
        case MODE_POST_FILTER:
            omp_set_num_threads(1);   /* see get_cur_ms() */
            load_map(s, q);
            s.post_filter();
            put_mat("post_filter", s.filtered_disp);
            break;
        case MODE_COLORMAP:
            load_map(s, q);
            s.colormap();
            put_mat("colormap", s.colored_disp);
            break;
        default:
            need(false, "mode");
        }
    }
    if (fclose(g_out) != 0)
        return 2;
    return 0;
}
