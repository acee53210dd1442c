// Scene::saveAsNVM end to end (BASELINE.json configs[0], "tiny nvm scene"): read an NVM_V3 model whose cameras point at
// binary PPM images, build the Scene as run_nvm_scene does, refine the seeds, write the scene with saveAsNVM and check
// what was written: project.nvm reads back through NVMReader::readFile with the right counts, r == 0, unit quaternions
// whose rotation has the cameras' normalised axes as rows, every point's centre, colour and measurements, and a Scene built
// from the written folder loads (its views are the written JPEG files); Image::saveJpeg writes view 0's pixels beside it.
// The files' bytes are compared by the Python test.
//   save_as_nvm_cpp <in.nvm> <out folder> <start_level>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <hpmvs/HpmvsOptions.h>
#include <hpmvs/NVMReader.h>
#include <hpmvs/Scene.h>

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "check failed: " __VA_ARGS__); \
            fprintf(stderr, "\n");                        \
            return 10;                                    \
        }                                                 \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<mo3d::NVM_Model> models;
    mo3d::NVMReader::readFile(argv[1], models, true);
    if (models.empty()) { fprintf(stderr, "no model\n"); return 3; }
    mo3d::HpmvsOptions options;
    options.START_LEVEL = atoi(argv[3]);
    mo3d::Scene scene;
    if (!scene.addCameras(models[0], options)) { fprintf(stderr, "addCameras failed\n"); return 4; }
    if (!scene.extractCoVisiblilty(models[0], options)) return 5;
    std::vector<mo3d::Ppatch3d> patches;
    if (!scene.initPatches(models[0], options, patches)) { fprintf(stderr, "initPatches failed\n"); return 6; }
    if (!scene.saveAsNVM(argv[2], patches)) { fprintf(stderr, "saveAsNVM failed\n"); return 7; }

    // Image::saveJpeg of a view that holds pixels (k1 == 0 here: the Python test compares the file with level 0's)
    if (!scene.images_[0].saveJpeg((std::string(argv[2]) + "/view0_pixels.jpg").c_str())) { fprintf(stderr, "saveJpeg failed\n"); return 7; }
    if (scene.images_[0].saveJpeg((std::string(argv[2]) + "/refused.jpg").c_str(), 0)) { fprintf(stderr, "saveJpeg took quality 0\n"); return 7; }
    const std::string nvm = std::string(argv[2]) + "/project.nvm";
    std::vector<mo3d::NVM_Model> back;
    mo3d::NVMReader::readFile(nvm.c_str(), back, true);
    CHECK(back.size() == 1, "%zu models read back", back.size());
    const mo3d::NVM_Model& m = back[0];
    CHECK(m.cameras.size() == scene.cameras_.size(), "%zu cameras", m.cameras.size());
    CHECK(m.points.size() == patches.size(), "%zu points for %zu patches", m.points.size(), patches.size());
    double worst_norm = 0.0, worst_row = 0.0;
    for (size_t i = 0; i < m.cameras.size(); i++) {
        const mo3d::NVM_Camera& c = m.cameras[i];
        const mo3d::Camera& cam = scene.cameras_[i];
        CHECK(c.r == 0.0, "camera %zu: r = %g", i, c.r);
        CHECK((float)c.f == cam.kMat_[0](0, 0), "camera %zu: f = %.9g", i, c.f);
        for (int k = 0; k < 3; k++)
            CHECK((float)c.c[k] == (float)((double)cam.center_[k] / (double)cam.center_[3]), "camera %zu: centre[%d] = %.9g", i, k, c.c[k]);
        const double w = c.rq[0], x = c.rq[1], y = c.rq[2], z = c.rq[3];
        // (the file holds 12 significant digits: each component is off by at most 5e-13 of itself, and so is the norm)
        worst_norm = std::fmax(worst_norm, std::fabs(std::sqrt(w * w + x * x + y * y + z * z) - 1.0));
        const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                                {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                                {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
        const Eigen::Vector3f ax[3] = {cam.xAxis_.normalized(), cam.yAxis_.normalized(), cam.zAxis_.normalized()};
        for (int r = 0; r < 3; r++)
            for (int k = 0; k < 3; k++) worst_row = std::fmax(worst_row, std::fabs(R[r][k] - (double)ax[r][k]));
    }
    CHECK(worst_norm <= 1e-12, "a quaternion's norm differs from 1 by %.3g", worst_norm);
    CHECK(worst_row <= 1e-6, "rotation rows differ from the axes by %.3g", worst_row);
    size_t n_meas = 0;
    for (size_t i = 0; i < patches.size(); i++) {
        const mo3d::Patch3d& p = *patches[i];
        const mo3d::NVM_Point& q = m.points[i];
        for (int k = 0; k < 3; k++) {
            CHECK((float)q.xyz[k] == (float)((double)p.center_[k] / (double)p.center_[3]), "point %zu: centre[%d] = %.9g", i, k, q.xyz[k]);
            CHECK((int)q.rgb[k] == (int)p.color_[k], "point %zu: colour[%d] = %g", i, k, q.rgb[k]);
        }
        CHECK(q.measurements.size() == p.images_.size(), "point %zu: %zu measurements", i, q.measurements.size());
        for (size_t j = 0; j < p.images_.size(); j++) {
            const mo3d::NVM_Measurement& me = q.measurements[j];
            CHECK(me.imgIndex == p.images_[j] && me.featIndex == 0, "point %zu: measurement %zu names image %d", i, j, me.imgIndex);
            const Eigen::Vector3f xy = scene.cameras_[me.imgIndex].project(p.center_, 0);
            CHECK((float)me.xy[0] == xy[0] && (float)me.xy[1] == xy[1], "point %zu: measurement %zu at %.9g %.9g", i, j, me.xy[0], me.xy[1]);
            n_meas++;
        }
    }
    // the written folder is a dataset this library loads: the views are baseline 4:2:0 files its decoder accepts
    mo3d::Scene again;
    if (!again.addCameras(m, options)) { fprintf(stderr, "addCameras of the written folder failed\n"); return 8; }
    if (!again.extractCoVisiblilty(m, options)) return 8;
    for (size_t i = 0; i < again.images_.size(); i++) {
        CHECK(again.images_[i].isJpeg(), "view %zu of the written folder is no JPEG", i);
        CHECK(again.images_[i].getWidth() == scene.images_[i].getWidth() && again.images_[i].getHeight() == scene.images_[i].getHeight(),
              "view %zu: %d x %d", i, again.images_[i].getWidth(), again.images_[i].getHeight());
    }
    if (!again.deviceScene()) { fprintf(stderr, "the written folder does not upload\n"); return 9; }
    printf("cameras %zu points %zu measurements %zu quaternion_norm_error %.3e row_error %.3e reloaded %zu\n", m.cameras.size(), m.points.size(),
           n_meas, worst_norm, worst_row, again.images_.size());
    return 0;
}
