// rle_build.h — which kind of build this is (the Makefile sets it; the product library does not).
//   RLE_TEST_HOOKS  1: the drop-in's fault-injection and fake-device hooks (test library, the CPU
//                   lifecycle builds).
#pragma once
#ifndef RLE_TEST_HOOKS
#define RLE_TEST_HOOKS 0
#endif
