// Derived weights of the model loaders: the plane copies of a packed fp32 [rows][K] matrix that is already on the device, in memory the
// model owns.  One path for ResNet-50 (resnet50.hip, conv1_x6.hip), VGG-16 (vgg16.hip) and the ViT's split planes (vit.hip).
#include "relax_internal.h"

namespace relax {

int derive_sp3(relax_handle* h, DeviceOwner& mem, const float* w_dev, int rows, int K, void** out, const char* what) {
    *out = mem.keep(h, (size_t)rows * K * 6, what);
    if (!*out) return RELAX_ERR_NOMEM;
    return launch_to_sp3(h, w_dev, K, *out, rows, K, nullptr);
}

int derive_h2_rows(relax_handle* h, DeviceOwner& mem, const float* w_dev, int rows, int K, void** planes, float** inv, const char* what) {
    *planes = mem.keep(h, (size_t)rows * K * 4, what);
    *inv = *planes ? static_cast<float*>(mem.keep(h, sizeof(float) * (size_t)rows, what)) : nullptr;
    if (!*inv) return RELAX_ERR_NOMEM;
    return launch_to_h2_rows(h, w_dev, K, *planes, rows, K, *inv, nullptr);
}

}  // namespace relax
