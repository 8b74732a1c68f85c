// The zigzag scan of an 8 x 8 block (ITU-T T.81 figure 5): entry k is the natural (row-major) index of zigzag position k.  One
// initialiser list for every table of it: the encoder's host and constant tables (trl_jpeg.hip), the decoder's parser table
// (trl_jpegd_parse.h) and its constant table (trl_jpegd.hip); each declares its own element type and alignment.  Plain C: the
// parser header is also compiled into host-only programs (tests/jpegd_fuzz.cpp).
#ifndef TRL_ZIGZAG_H
#define TRL_ZIGZAG_H
#define TRL_ZIGZAG_LIST                                                                                                       \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
#endif
