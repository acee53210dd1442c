// mo3d::Image -- the level-0 pixels of one view (reference include/hpmvs/Image.h:50-87).  The reference
// loads a JPEG through CImg, undistorts it when the camera's radial coefficient k1 (NVM field r) is not 0
// and builds the pyramid on the host (src/hpmvs/Image.cpp:41-146); here the caller hands over interleaved
// u8 RGB, or the view is a baseline JPEG file as VisualSFM's NVM names it, whose bytes are kept and decoded on
// the GPU (hpmvs_scene_set_view_jpeg); both the undistortion and the pyramid run on the GPU when the scene is
// uploaded (Scene::deviceScene: hpmvs_scene_set_view_distorted for raw pixels).
#ifndef HPMVS_IMAGE_H_
#define HPMVS_IMAGE_H_
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include <hpmvs/NVMReader.h>
namespace mo3d {
class Image {
public:
    Image() : f_(1.0f), k1_(0.0f), maxLevel_(0), width_(0), height_(0), raw_(false) {}
    virtual ~Image() {}
    void init(const mo3d::NVM_Camera* cam, const int maxLevel = 1);
    // The file's first bytes decide: FF D8 is a JPEG, "P6" a binary PPM (the reference and CImg go by the extension).  A PPM's
    // pixels are kept raw (as the camera recorded them).  Of a JPEG the file's bytes are kept and width and height are taken
    // from hpmvs_jpeg_info, which refuses what the decoder would refuse (include/hpmvs_amd.h); no pixel is decoded here.
    bool load();
    // the same for a JPEG file the caller holds in memory; false (and the image unchanged) for a file that is refused
    bool setJpeg(const uint8_t* bytes, size_t n);
    bool isJpeg() const { return !jpeg_.empty(); }
    const std::vector<uint8_t>& jpegBytes() const { return jpeg_; }
    // pixels taken as given: already undistorted (or k1 == 0); k1 is NOT applied to them
    void setPixels(int width, int height, const uint8_t* rgb_interleaved);
    // pixels as the camera recorded them: undistorted with f and k1 on upload when k1 != 0
    void setRawPixels(int width, int height, const uint8_t* rgb_interleaved);
    bool isRaw() const { return raw_; }
    float getFocal() const { return f_; }  // Image::f_ (float, NVM f)
    float getK1() const { return k1_; }    // Image::k1_ (float, NVM r)
    inline int getWidth(int level = 0) const { return width_ >> level; }
    inline int getHeight(int level = 0) const { return height_ >> level; }
    int levels() const { return maxLevel_ + 1; }
    // level-0 pixels; of a JPEG image they are decoded on first use (hpmvs_jpeg_decode on device 0; empty when that fails)
    const std::vector<uint8_t>& pixels() const;
    // the pixels the image holds (pixels()) as the baseline JPEG file the reference's CImg save writes through libjpeg's
    // defaults, byte for byte (hpmvs_jpeg_encode on device 0: YCbCr 4:2:0, standard Huffman tables; CImg's quality is 100).
    // False, with the reason on stderr, for an image without pixels, a refused size or quality, or a file that cannot be written.
    bool saveJpeg(const char* path, int quality = 100) const;
private:
    mutable std::vector<uint8_t> rgb_;
    std::vector<uint8_t> jpeg_;  // the file, when the view is a JPEG
    std::string path_;
    float f_, k1_;
    int maxLevel_, width_, height_;
    bool raw_;  // rgb_ still carries the radial distortion
};
}  // namespace mo3d
#endif
