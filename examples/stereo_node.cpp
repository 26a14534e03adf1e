// stereo_node.cpp -- the reference ROS node's per-frame flow (node.cpp:25-151)
// on libsgm_hip.so through the drop-in headers, without ROS or OpenCV:
//
//   images (8-bit PGM, or PPM)    node.cpp:69-70   imread(..., IMREAD_GRAYSCALE); a colour pair's
//                                                  conversion runs on the GPU (set_input_format)
//   resize to img_w x img_h       node.cpp:75-78   cv::resize on the GPU (HipSolver::resize)
//   or rectify (MAPS.f32)         (not in the node) cv::remap on the GPU (HipSolver::set_rectify)
//   sky masks, both views         node.cpp:80-87   SkyAreaDetector::detect
//   SGM(h, w, s, d).process       node.cpp:49,93   (both views, LR check, post_filter)
//   get_disp()                    node.cpp:104     -> OUT_disp.f32 (raw float32 rows)
//   show_disp(debug_view)         node.cpp:107-110 -> OUT_debug.ppm (the node's imwrite)
//   point cloud                   node.cpp:113-143 -> OUT_cloud.bin (N x 3 float64 + N u8)
//   reprojection (Q.f64)          (not in the node) -> OUT_xyz.f32, OUT_depth.f32 (set_reproject)
//
// The configured size (node.cpp:19-20 g_img_w, g_img_h) is the images' size
// unless img_w img_h are given: then the solver is built at that size and both
// images are resized to it as node.cpp:75-76 does, on the GPU, before the sky
// detector, the matcher and the point cloud see them.  The calibration
// (read_calib, utils.cpp:59-89) comes from the command line.  Every stage runs
// on the GPU.
// With MAPS.f32 -- four dense img_h x img_w float32 planes x_l, y_l, x_r, y_r,
// cv::initUndistortRectifyMap's CV_32FC1 outputs for both views -- the images
// are raw camera images and are rectified instead of resized: the sky detector
// sees HipSolver::remap's images, process() takes the raw pair and every frame
// begins with the remap, and the cloud reads the rectified left image.
//
// LEFT and RIGHT may be binary PPM files (P6, maxval 255) instead: they are read
// as RGB8, the solver's input format is set to SGM_PIX_RGB8 and process() takes
// the colour pair -- every frame converts it on the GPU, inside the resize or
// the remap when one is on.  The sky detector sees HipSolver::gray's images, the
// debug view and the cloud read the grey image the frame matched.
//
// With max_range Q.f64 -- stereoRectify's 4 x 4 Q as 16 doubles, row-major, the
// fifteenth argument, after the range beyond which a depth is missing (0: none)
// -- every frame also reprojects its map on the GPU, and the node writes the
// organized XYZ image (float32 x 3 per pixel, NaN where missing) and the depth
// image (float32) it would publish as PointCloud2 and sensor_msgs/Image 32FC1
// (INTEGRATION.md).  In that form img_w img_h may be 0 0 (the images' size) and
// MAPS.f32 may be - (no maps).
//
// usage: stereo_node LEFT.pgm RIGHT.pgm OUT_PREFIX
//                    [scale max_disp [fx fy cx cy [min_disp [img_w img_h [MAPS.f32 [max_range Q.f64]]]]]]
// min_disp (not in the node): search disparities [min_disp, min_disp + max_disp);
// the map, the debug view and the cloud are then in true disparity.
#include "sgm_amd/SGM.h"
#include "sgm_amd/SkyAreaDetector.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

using sgm_amd::Mat;
typedef std::shared_ptr<sky_detector::SkyAreaDetector> SkyDetPtr;  // node.cpp:8

// binary PGM (P5, maxval 255) -> CV_8UC1; binary PPM (P6, maxval 255) -> CV_8UC3 in RGB order
static bool read_pgm(const std::string &path, Mat &img) {
    std::ifstream f(path, std::ios::binary);
    std::string magic;
    int w = 0, h = 0, maxval = 0;
    if (!(f >> magic >> w >> h >> maxval) || (magic != "P5" && magic != "P6") || maxval != 255 || w <= 0 ||
        h <= 0)
        return false;
    f.get();  // the single whitespace after maxval
    const int ch = magic == "P6" ? 3 : 1;
    img.create(h, w, ch == 3 ? CV_8UC3 : CV_8UC1);
    for (int i = 0; i < h; ++i) f.read(reinterpret_cast<char *>(img.ptr<unsigned char>(i)), (std::streamsize)w * ch);
    return (bool)f;
}

static bool write_ppm(const std::string &path, const Mat &bgr) {
    std::ofstream f(path, std::ios::binary);
    f << "P6\n" << bgr.cols << " " << bgr.rows << "\n255\n";
    std::vector<unsigned char> row((size_t)bgr.cols * 3);
    for (int i = 0; i < bgr.rows; ++i) {
        const unsigned char *p = bgr.ptr<unsigned char>(i);
        for (int j = 0; j < bgr.cols; ++j) {  // BGR -> RGB
            row[3 * j] = p[3 * j + 2];
            row[3 * j + 1] = p[3 * j + 1];
            row[3 * j + 2] = p[3 * j];
        }
        f.write(reinterpret_cast<const char *>(row.data()), (std::streamsize)row.size());
    }
    return (bool)f;
}

int main(int argc, char **argv) {
    if (argc != 4 && argc != 6 && argc != 10 && argc != 11 && argc != 13 && argc != 14 && argc != 16) {
        std::fprintf(stderr,
                     "usage: %s LEFT.pgm RIGHT.pgm OUT_PREFIX "
                     "[scale max_disp [fx fy cx cy [min_disp [img_w img_h [MAPS.f32 [max_range Q.f64]]]]]]\n",
                     argv[0]);
        return 2;
    }
    const std::string out = argv[3];
    const int scale = argc > 4 ? std::atoi(argv[4]) : 1;        // node.cpp:21 g_scale
    const int max_disp = argc > 5 ? std::atoi(argv[5]) : 128;   // node.cpp:22 g_max_disp
    sgm_camera cam;                                             // KITTI image_0 defaults
    cam.fx = argc > 6 ? (float)std::atof(argv[6]) : 721.5377f;
    cam.fy = argc > 7 ? (float)std::atof(argv[7]) : 721.5377f;
    cam.cx = argc > 8 ? (float)std::atof(argv[8]) : 609.5593f;
    cam.cy = argc > 9 ? (float)std::atof(argv[9]) : 172.854f;
    const int min_disp = argc > 10 ? std::atoi(argv[10]) : 0;   // sgm_set_min_disp
    cam.baseline = 0.5;    // node.cpp:123
    cam.max_range = 100;   // node.cpp:122

    Mat img_l, img_r;
    if (!read_pgm(argv[1], img_l) || !read_pgm(argv[2], img_r) || img_l.rows != img_r.rows ||
        img_l.cols != img_r.cols || img_l.type() != img_r.type()) {
        std::fprintf(stderr, "cannot read two 8-bit PGM images of one size\n");
        return 2;
    }
    // node.cpp:19-20 g_img_w, g_img_h (default: the images' size, nothing to resize)
    // (with a Q.f64: 0 0 = the images' size, and - for MAPS.f32 = no maps)
    const bool sized = argc > 12 && !(argc > 15 && std::atoi(argv[11]) == 0 && std::atoi(argv[12]) == 0);
    const bool rectify = argc > 13 && !(argc > 15 && std::string(argv[13]) == "-");
    const int w = sized ? std::atoi(argv[11]) : img_l.cols;
    const int h = sized ? std::atoi(argv[12]) : img_l.rows;
    std::printf("left size: %d, %d\nright size: %d, %d\n", img_l.rows, img_l.cols, img_r.rows,
                img_r.cols);

    // node.cpp:49-51
    sgm_amd::SolverPtr sv = std::make_shared<sgm_amd::SGM>(h, w, scale, max_disp, 8, min_disp);
    SkyDetPtr sky_det = std::make_shared<sky_detector::SkyAreaDetector>();

    Mat raw_l = img_l, raw_r = img_r;  // what process() takes
    const bool colour = img_l.type() == CV_8UC3;
    if (colour) {  // a P6 pair: the frame converts it; img_l, img_r (grey) are for the sky detector
        sgm_amd::SGM *sgm = static_cast<sgm_amd::SGM *>(sv.get());
        sgm->set_input_format(SGM_PIX_RGB8);
        sgm->gray(raw_l, img_l, SGM_PIX_RGB8);
        sgm->gray(raw_r, img_r, SGM_PIX_RGB8);
    }
    if (rectify) {  // rectify instead: the maps are at the configured size
        sgm_amd::SGM *sgm = static_cast<sgm_amd::SGM *>(sv.get());
        Mat maps[4];
        std::ifstream f(argv[13], std::ios::binary);
        for (Mat &m : maps) {
            m.create(h, w, CV_32FC1);
            f.read(reinterpret_cast<char *>(m.data), (std::streamsize)h * w * 4);
        }
        if (!f || f.peek() != std::ifstream::traits_type::eof()) {
            std::fprintf(stderr, "%s does not hold four %d x %d float32 planes\n", argv[13], h, w);
            return 2;
        }
        sgm->set_rectify(img_l.rows, img_l.cols, maps[0], maps[1], maps[2], maps[3]);
        sgm->remap(img_l, img_l, 0);  // for the sky detector; the frame remaps the raw pair itself
        sgm->remap(img_r, img_r, 1);
        std::printf("rectified left size: %d, %d\n", img_l.rows, img_l.cols);
        std::printf("rectified right size: %d, %d\n", img_r.rows, img_r.cols);
    } else if (sized) {  // node.cpp:75-78, on the GPU
        sgm_amd::SGM *sgm = static_cast<sgm_amd::SGM *>(sv.get());
        if (colour) sgm->set_input_size(img_l.rows, img_l.cols);  // (the frame resizes the colour pair itself)
        sgm->resize(img_l, img_l);
        sgm->resize(img_r, img_r);
        std::printf("resized left size: %d, %d\n", img_l.rows, img_l.cols);
        std::printf("resized right size: %d, %d\n", img_r.rows, img_r.cols);
        if (!colour) {
            raw_l = img_l;
            raw_r = img_r;
        }
    }

    if (argc > 15) {  // max_range Q.f64: XYZ and depth of every frame's map, on the GPU
        double q[16];
        std::ifstream f(argv[15], std::ios::binary);
        if (!f.read(reinterpret_cast<char *>(q), sizeof(q)) || f.peek() != std::ifstream::traits_type::eof()) {
            std::fprintf(stderr, "%s does not hold 16 float64 values\n", argv[15]);
            return 2;
        }
        static_cast<sgm_amd::SGM *>(sv.get())->set_reproject(q, SGM_REPROJECT_XYZ | SGM_REPROJECT_DEPTH,
                                                                 (float)std::atof(argv[14]));
    }

    Mat sky_mask, sky_mask_beta;  // node.cpp:80-87 (no debug image is written)
    sky_det->detect(img_l, out + "_sky.png", sky_mask, scale);
    sky_det->detect(img_r, out + "_sky2.png", sky_mask_beta, scale);

    const auto be = std::chrono::steady_clock::now();
    sv->process(raw_l, raw_r, sky_mask, sky_mask_beta);  // node.cpp:93
    const auto en = std::chrono::steady_clock::now();
    std::printf("stereo matching done\ntime cost: %lf ms\n",
                std::chrono::duration<double, std::milli>(en - be).count());

    const Mat &disp = sv->get_disp();  // node.cpp:104
    {
        std::ofstream f(out + "_disp.f32", std::ios::binary);
        for (int i = 0; i < disp.rows; ++i)
            f.write(reinterpret_cast<const char *>(disp.ptr<float>(i)), (std::streamsize)disp.cols * 4);
    }
    if (argc > 15) {  // what the node would publish as PointCloud2 (organized) and Image 32FC1
        const sgm_amd::SGM *sgm = static_cast<sgm_amd::SGM *>(sv.get());
        std::ofstream fx(out + "_xyz.f32", std::ios::binary), fd(out + "_depth.f32", std::ios::binary);
        for (int i = 0; i < disp.rows; ++i) {
            fx.write(reinterpret_cast<const char *>(sgm->xyz().ptr<float>(i)), (std::streamsize)disp.cols * 12);
            fd.write(reinterpret_cast<const char *>(sgm->depth().ptr<float>(i)), (std::streamsize)disp.cols * 4);
        }
        if (!fx || !fd) return 3;
    }
    Mat debug_view;  // node.cpp:107-110
    sv->show_disp(debug_view);
    if (!write_ppm(out + "_debug.ppm", debug_view)) return 3;

    // node.cpp:113-143: the cloud in row-major push_back order, on the GPU
    // (sgm_stage_point_cloud) through the solver's handle
    const size_t npx = (size_t)disp.rows * disp.cols;
    std::vector<double> xyz(3 * npx);
    std::vector<unsigned char> pix(npx);
    int n = 0;
    Mat packed = disp.clone();
    if (rectify) img_l = static_cast<sgm_amd::SGM *>(sv.get())->rectified(0);  // what the frame matched
    else if (colour) img_l = static_cast<sgm_amd::SGM *>(sv.get())->input_gray(0);
    const int rc = sgm_stage_point_cloud(static_cast<sgm_amd::SGM *>(sv.get())->handle(),
                                         packed.ptr<float>(0), img_l.data, (int)img_l.step, &cam,
                                         xyz.data(), pix.data(), &n);
    if (rc != SGM_OK) {
        std::fprintf(stderr, "point cloud: %s\n",
                     sgm_last_error(static_cast<sgm_amd::SGM *>(sv.get())->handle()));
        return 4;
    }
    std::printf("pointcloud size: %d, %d\n", n, n);
    std::ofstream f(out + "_cloud.bin", std::ios::binary);
    f.write(reinterpret_cast<const char *>(xyz.data()), (std::streamsize)n * 3 * sizeof(double));
    f.write(reinterpret_cast<const char *>(pix.data()), (std::streamsize)n);
    return f ? 0 : 3;
}
