// Leaf-test build of rd_kernel_tools.hip (lib/libhevcdl_hip_leaf.so, -DHEVCDL_LEAF_TEST; test infrastructure): the kernel's translation unit with the leaf harness behind it.
#include "rd_kernel_tools.hip"
#include "rd_leaf_harness.h"
