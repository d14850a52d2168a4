// Leaf-test build of rd_kernel_bd10.hip (lib/libhevcdl_hip_leaf.so, -DHEVCDL_LEAF_TEST; test infrastructure): the kernel's translation unit with the leaf harness behind it.
#include "rd_kernel_bd10.hip"
#include "rd_leaf_harness.h"
